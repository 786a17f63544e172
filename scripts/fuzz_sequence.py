#!/usr/bin/env python
"""ONE long-lived net against the float64 oracle across steps of changing shape (test infrastructure, like tests/).

scripts/fuzz_step.py builds a fresh net for every case and takes one step: zero Adam moments, clock 0, workspaces that have
just been allocated zeroed.  Here a net is built and loaded ONCE and then runs SCHEDULE: seven training steps and two
scorings over four shapes of one family (A twice, the larger B, an evaluation feed E of another group size, A again after B,
the smallest C, E again, A, B), so that every workspace is used a second time, stale after another shape, the Adam clock and
moments are live, rows touched earlier are not touched now, and launch plans are recorded and replayed.

TEACHER FORCING.  Before every step the net's ``state_dict()`` is read -- variables, batch-norm moving statistics, Adam
moments, clock -- and the float64 oracle takes its step FROM THAT STATE (``step = clock + 1``).  Both sides start every step
from the same numbers, so the single-step bars of fuzz_step / tests/test_step_gpu.py apply unchanged at every step and
Adam's habit of turning a noise-level gradient into a +-lr step never accumulates into drift.  Nothing is loaded into the
net after construction.

    python scripts/fuzz_sequence.py [clsr,gru4rec,din,sli_rec,a2svd,dien,caser,ncf,nextitnet]
    FUZZ_F32=cpu python scripts/fuzz_sequence.py ...     no GPU: the float32 ORACLE takes the net's place, teacher-forced the
                                                         same way, and must meet every bar; ends with the worst ratio per bar
    FUZZ_PRECISION=fp32x3                                the CLSR sequences in the two-piece product mode

Two passes on the GPU: pass 1 with launch plans and one persistent uploaded feed object per shape (shape A is recorded at its
second step and replayed at the third and fourth; a scoring runs its forward twice, so that the second scoring replays the
plan the first one recorded), pass 2 on a new net without plans and with captured gradients, which are then held to the
oracle as well (fuzz_step.table_checks' bars), so that a failure names a gradient rather than an update.
"""
import copy
import os
import sys
import traceback
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_step as FS  # noqa: E402
from fuzz_step import STATS, close  # noqa: E402
from bench import build_hparams  # noqa: E402
from oracle import clsr_oracle as O  # noqa: E402
from oracle import sibling_oracle as SO  # noqa: E402

BETA1, BETA2 = 0.9, 0.999
EPS32 = 2.0 ** -23
# The bar of the m increment is the derived one, (1 - beta1) times the gradient bar.  The derived bar of the v increment,
# (1 - beta2) (4e-3 g^2 + 2 |g| a + a^2), is MISSED by the float32 oracle (by up to 1.2e4 on a dense variable):
# v' is stored in float32 and formed by about four roundings of 2^-24 (the float32 beta2, two products, one sum), and
# (1 - beta2) g^2 of a gradient a tenth of the earlier ones is below ONE such rounding of beta2 v.  So the v bar alone
# carries V_ROUND |v'| on top: the float32 oracle's worst error is 0.98 * 2^-23 |v'|, held at the factor of two that the
# gradient bars keep over their float32 worst case.
V_ROUND = 2 * EPS32
# Rows NOT touched at a P = 1 step, dense Adam: gradient exactly zero on both sides, the moment is beta times the old one,
# two roundings (the float32 beta, the product); compared whole at 2 * 2^-23 relative, since the gradient bars are skipped
DECAY_ROUND = 2 * EPS32

# (what, shape, variant): the variant picks the feed seed -- other ids at the same shape
SCHEDULE = (("train", "A", 0), ("train", "A", 1), ("train", "B", 0), ("score", "E", 0), ("train", "A", 2),
            ("train", "C", 0), ("score", "E", 0), ("train", "A", 3), ("train", "B", 1))
SEQ_SEED = 2024
CLSR_KINDS = ("clsr",)
SIB_KINDS = ("gru4rec", "din", "sli_rec", "a2svd", "dien")
OWN_KINDS = ("caser", "ncf", "nextitnet")
VOCAB = dict(Vu=50, Vi=200, Vc=12)


# ------------------------------------------------------------------------------------------ model families
def _tests_on_path():
    t = os.path.join(ROOT, "tests")
    if t not in sys.path:
        sys.path.insert(0, t)


class Family(object):
    """What differs between the model families: the oracle's entry points, the tables and their clip-norm slots, how a net
    is built.  ``train`` / ``predict`` have one signature for all (NCF's oracle has no batch-norm state)."""
    loss_keys = ("loss", "data_loss", "regular_loss")
    # P = 1: every row of the batch is identical and batch-norm outputs sit on the ReLU kink; NCF has no batch norm, but its
    # P = 1 gradients are at most 4e-7 (the user-table ones cancel to 1e-18) and decided by float32 rounding all the same
    p1_comparable = False

    def __init__(self, kind):
        self.kind = kind

    def touched(self, feed):
        return O.touched_rows(feed, self.tmap)

    def init_bn(self, params):
        return O.init_bn_state(params)


class ClsrFamily(Family):
    loss_keys = ("loss", "data_loss", "regular_loss", "contrastive_loss", "discrepancy_loss")
    tmap = O.TABLES
    norm_slots = dict(item=(0, 2, 4), cate=(1, 3, 5), user_long=(6, 8), user_short=(7, 9))
    user_tables = ("user_long", "user_short")

    def init_params(self, dims, hp, seed):
        return O.init_params(dims, hp, seed=seed, scale_dense=8.0)

    def train(self, p, bn, adam, step, tf, hp, lazy, group=None):
        return O.train_step(p, bn, adam, step, tf, hp, lazy=lazy, dedup_group=group)

    def predict(self, p, bn, tf, hp):
        return O.predict(p, bn, tf, hp)

    def make_net(self, hp, dims, dedup, precision):
        from clsr_amd.net import CLSRNet
        return CLSRNet(hp, dims, device="cuda:0", seed=0, dedup_histories=dedup, precision=precision)


class SibFamily(Family):
    tmap = SO.TABLES
    norm_slots = dict(item=(0, 2, 4), cate=(1, 3, 5))
    user_tables = ()

    def init_params(self, dims, hp, seed):
        return SO.init_params(dims, hp, self.kind, seed=seed, scale_dense=8.0)

    def train(self, p, bn, adam, step, tf, hp, lazy, group=None):
        return SO.train_step(p, bn, adam, step, tf, hp, self.kind, lazy=lazy, dedup_group=group)

    def predict(self, p, bn, tf, hp):
        return SO.predict(p, bn, tf, hp, self.kind)

    def make_net(self, hp, dims, dedup, precision):
        from clsr_amd.seqnet import SeqNet
        return SeqNet(hp, dims, kind=self.kind, device="cuda:0", seed=0, dedup_histories=dedup)


class OwnFamily(SibFamily):
    """Caser, NCF, NextItNet: the oracles under tests/."""

    def __init__(self, kind):
        Family.__init__(self, kind)
        _tests_on_path()
        if kind == "caser":
            import caser_oracle as M
        elif kind == "ncf":
            import ncf_oracle as M
            self.tmap = M.TABLES
            self.norm_slots = dict(item=(4,), cate=(5,), user_gmf=(6,), user_mlp=(7,), item_gmf=(8,), item_mlp=(9,))
            self.user_tables = ("user_gmf", "user_mlp", "item_gmf", "item_mlp")
        else:
            import nextitnet_oracle as M
            self.p1_comparable = True       # one history still gives T G different rows
        self.M = M

    def init_params(self, dims, hp, seed):
        return self.M.init_params(dims, hp, **dict(self.M.FIXTURE, seed=seed))

    def init_bn(self, params):
        return OrderedDict() if self.kind == "ncf" else O.init_bn_state(params)

    def touched(self, feed):
        if self.kind != "ncf":
            return O.touched_rows(feed, self.tmap)
        rows = O.touched_rows(feed, dict(item=self.tmap["item"], cate=self.tmap["cate"]))
        ids = lambda k: torch.unique(torch.as_tensor(np.asarray(feed[k])).reshape(-1).long())
        for key in self.M.NCF_KEYS:
            rows[self.tmap[key]] = ids("users" if key.startswith("user") else "items")
        return rows

    def train(self, p, bn, adam, step, tf, hp, lazy, group=None):
        if self.kind == "ncf":          # (its own four tables take the norm of the un-merged slices in either mode)
            new_p, new_a, ls, grads, norms, out = self.M.train_step(p, adam, step, tf, hp, lazy=lazy)
            return new_p, OrderedDict(), new_a, ls, grads, norms, out
        if self.kind == "caser":
            return self.M.train_step(p, bn, adam, step, tf, hp, lazy=lazy, dedup_group=group)
        return self.M.train_step(p, bn, adam, step, tf, hp, lazy=lazy)

    def predict(self, p, bn, tf, hp):
        return self.M.predict(p, tf, hp) if self.kind == "ncf" else self.M.predict(p, bn, tf, hp)

    def make_net(self, hp, dims, dedup, precision):
        from clsr_amd.seqnet import SeqNet
        kw = {} if self.kind == "nextitnet" else dict(dedup_histories=dedup)
        return SeqNet(hp, dims, kind=self.kind, device="cuda:0", seed=0, **kw)


def family(kind):
    return ClsrFamily(kind) if kind == "clsr" else (SibFamily(kind) if kind in SIB_KINDS else OwnFamily(kind))


# ------------------------------------------------------------------------------------------ the committed sequences
def _seq(sid, kind, hp, dims, dedup, shapes, feed_of, seeds=None, note=""):
    """``shapes``: name -> dict(P, T, G); ``feed_of(shape name, shape, seed)`` -> numpy feed; ``seeds``: (shape, variant) ->
    feed seed where the default one (feed_seed) fails the input conditions."""
    s = types.SimpleNamespace(id=sid, kind=kind, hp=hp, dims=dims, dedup=dedup, shapes=shapes, feed_of=feed_of,
                              seeds=dict(seeds or {}), lazy=str(hp.optimizer).lower() == "lazyadam", _feeds={})
    s.desc = "%s [%s, dedup=%s, %s] %s" % (sid, hp.optimizer, dedup, " ".join(
        "%s:P%d,T%d,G%d" % (n, sh["P"], sh["T"], sh["G"]) for n, sh in sorted(shapes.items())), note)
    return s


def feed_seed(s, shape, variant):
    return s.seeds.get((shape, variant), 7000 + 100 * "ABCE".index(shape) + variant)


def group_of(s):
    """With de-duplicated histories the step takes a table's clip norm after summing the G slices of a group at the history
    and user-row sites (deliberate differences): the oracle is told, so that an ACTIVE clip scales alike."""
    return int(s.hp.train_num_ngs) + 1 if s.dedup and s.kind != "nextitnet" else None


def get_feed(s, shape, variant):
    key = (shape, variant)
    if key not in s._feeds:
        s._feeds[key] = s.feed_of(shape, s.shapes[shape], feed_seed(s, shape, variant))
    return s._feeds[key]


# CLSR: (encoder, optimizer, dedup, clip active, contrastive loss, length threshold, D, lengths, embed_l2, T = 65 at B)
CLSR_SEQS = (
    ("time4lstm", "adam", True, True, "triplet", 2, 16, "uniform", 1e-3, False),
    ("time4lstm", "lazyadam", False, False, "bpr", 5, 40, "uniform", 1e-6, False),
    ("gru", "lazyadam", True, True, "bpr", 2, 52, "uniform", 1e-3, False),
    ("gru", "adam", False, False, "triplet", 5, 16, "uniform", 1e-6, False),
    ("lstm", "adam", False, True, "bpr", 2, 40, "uniform", 1e-6, False),
    ("lstm", "lazyadam", True, False, "triplet", 5, 52, "uniform", 1e-3, True),     # A: T = 10, B: P = 3, T = 65
)
# Feed seeds replaced because the default one fails the input conditions (input_conditions: at every training step from the
# second on, the item table and every user table see a row that is new and lose one that was touched before); found on
# the CPU from the feeds alone: sequence id -> {(shape, variant): seed}
#
# Only step 6 (shape C, one positive: at most three item rows and ONE user row, which has to be new) ever needed another
# seed; ``python scripts/fuzz_sequence.py seeds`` prints this table (first of default, default + 1000, default + 2000, ...)
SEEDS = {
    "clsr-0-time4lstm": {("C", 0): 18200}, "clsr-1-time4lstm": {("C", 0): 18200}, "clsr-2-gru": {("C", 0): 37200},
    "clsr-3-gru": {("C", 0): 18200}, "clsr-4-lstm": {("C", 0): 37200}, "clsr-5-lstm": {("C", 0): 8200},
    "gru4rec-adam": {("C", 0): 16200}, "gru4rec-lazyadam": {("C", 0): 16200}, "din-adam": {("C", 0): 16200},
    "din-lazyadam": {("C", 0): 16200}, "sli_rec-adam": {("C", 0): 16200}, "sli_rec-lazyadam": {("C", 0): 16200},
    "a2svd-adam": {("C", 0): 16200}, "a2svd-lazyadam": {("C", 0): 16200}, "dien-adam": {("C", 0): 16200},
    "dien-lazyadam": {("C", 0): 16200}, "ncf-adam": {("C", 0): 29200}, "ncf-lazyadam": {("C", 0): 29200},
}


def _draw_feed(c):
    def feed_of(name, sh, seed):
        c2 = copy.copy(c)
        c2.T, c2.G = sh["T"], sh["G"]
        return FS.make_feed(c2, P=sh["P"], seed=seed)
    return feed_of


def clsr_sequences():
    out = []
    for i, (enc, opt, dedup, clip, closs, thr, D, lengths, el2, long_b) in enumerate(CLSR_SEQS):
        sid = "clsr-%d-%s" % (i, enc)
        pin = dict(D=D, T=10, P=7, G=int((3, 5, 2)[i % 3]), lengths=lengths, sequential_model=enc, optimizer=opt,
                   is_clip_norm=int(clip), max_grad_norm=0.01, contrastive_loss=closs, contrastive_length_threshold=thr,
                   contrastive_loss_weight=(0.1, 1.0)[i % 2], embed_l2=el2, discrepancy_loss_weight=(0.01, 0.5)[i % 2])
        c = FS.draw_case(np.random.default_rng([SEQ_SEED, i]), i, "clsr", pin=pin)
        shapes = dict(A=dict(P=7, T=10, G=c.G), B=dict(P=3, T=65, G=c.G) if long_b else dict(P=33, T=17, G=c.G),
                      C=dict(P=1, T=2, G=c.G), E=dict(P=5, T=10, G=c.G + 2))
        out.append(_seq(sid, "clsr", c.hp, c.dims, dedup, shapes, _draw_feed(c), SEEDS.get(sid), c.desc.split(": ", 1)[1]))
        out[-1].param_seed = i
    return out


def sibling_sequences(kinds=SIB_KINDS):
    out = []
    for k, kind in enumerate(SIB_KINDS):
        for j, opt in enumerate(("adam", "lazyadam")):
            if kind not in kinds:
                continue
            i = 10 + 2 * k + j
            sid = "%s-%s" % (kind, opt)
            pin = dict(T=10, P=7, G=int((3, 5)[(k + j) % 2]), lengths="uniform", optimizer=opt, is_clip_norm=int((k + j) % 2),
                       max_grad_norm=0.01)
            c = FS.draw_case(np.random.default_rng([SEQ_SEED, i]), i, kind, pin=pin)
            shapes = dict(A=dict(P=7, T=10, G=c.G), B=dict(P=33, T=17, G=c.G), C=dict(P=1, T=2, G=c.G),
                          E=dict(P=5, T=10, G=c.G + 2))
            out.append(_seq(sid, kind, c.hp, c.dims, bool(k % 2), shapes, _draw_feed(c), SEEDS.get(sid),
                            c.desc.split(": ", 1)[1]))
            out[-1].param_seed = i
    return out


# Caser / NCF / NextItNet at small admitted shapes of tests/{caser,ncf,nextitnet}_cases.py; T is part of the model (Caser's
# vertical filter, NextItNet's dilations against the history), so only P and the ids vary and shape C is P = 1
OWN_SHAPES = dict(
    caser=(dict(T=12, Di=8, Dc=4, G=3, over=dict(L=3, n_v=4, n_h=8)), dict(T=9, Di=4, Dc=4, G=5, over=dict(L=2, n_v=4, n_h=4))),
    ncf=(dict(T=5, Di=4, Dc=4, G=5, over=dict(user_embedding_dim=8, ncf_layer_sizes=[4])),
         dict(T=5, Di=4, Dc=4, G=2, over=dict(user_embedding_dim=4, ncf_layer_sizes=[36, 4]))),
    nextitnet=(dict(T=9, Di=4, Dc=4, G=3, over=dict(dilations=[1, 2], kernel_size=3)),
               dict(T=9, Di=4, Dc=4, G=5, over=dict(dilations=[4], kernel_size=3))),
)


def _synthetic_feed_of(dims):
    from clsr_amd.synthetic import synthetic_feed

    def feed_of(name, sh, seed):
        return synthetic_feed(sh["P"], sh["T"], dims["Vu"], dims["Vi"], dims["Vc"], G=sh["G"], lengths="uniform",
                              ids="uniform", seed=seed)
    return feed_of


def _nextitnet_feed_of(dims):
    def feed_of(name, sh, seed):
        import nextitnet_cases as XK        # (asks the built library for its limits: only once a NextItNet feed is drawn)
        lens = np.random.RandomState(seed).randint(1, sh["T"] + 1, sh["P"]).tolist()
        feed = XK.edge_feed(sh["T"], sh["G"], dims["Vi"], dims["Vc"], lens, seed=seed, Vu=dims["Vu"])
        if name == "E":         # a scoring feed holds the candidate of the last position only
            feed = dict(feed, **{k: np.ascontiguousarray(feed[k][:, -1:]) for k in ("items", "cates", "labels")})
        return feed
    return feed_of


def own_sequences(kinds=OWN_KINDS):
    out = []
    for k, kind in enumerate(OWN_KINDS):
        if kind not in kinds:
            continue
        fam = family(kind)
        for j, opt in enumerate(("adam", "lazyadam")):
            w = OWN_SHAPES[kind][j]
            cfg = dict(T=w["T"], Di=w["Di"], Dc=w["Dc"], Du=8, H=8, **VOCAB)
            hp = fam.M.hparams(build_hparams(cfg, 7, train_num_ngs=w["G"] - 1, optimizer=opt, is_clip_norm=int(j == 0),
                                             max_grad_norm=0.01 if kind != "ncf" else 0.05, layer_sizes=[16, 8]),
                               max_seq_length=w["T"], **w["over"])
            # NextItNet's targets are G ids at EVERY position: 33 histories of 9 steps draw ~900 of them, which leaves no row
            # of a 200-row item table untouched for the input conditions; its item table has 4000 rows instead
            dims = dict(VOCAB, Vi=4000) if kind == "nextitnet" else dict(VOCAB)
            cfg.update(dims)
            sid = "%s-%s" % (kind, opt)
            shapes = dict(A=dict(P=7, T=w["T"], G=w["G"]), B=dict(P=33, T=w["T"], G=w["G"]), C=dict(P=1, T=w["T"], G=w["G"]),
                          E=dict(P=5, T=w["T"], G=w["G"] + 2))
            feed_of = _nextitnet_feed_of(dims) if kind == "nextitnet" else _synthetic_feed_of(dims)
            out.append(_seq(sid, kind, hp, dims, bool(j), shapes, feed_of, SEEDS.get(sid), str(w["over"])))
            out[-1].param_seed = 30 + 2 * k + j
    return out


def sequences(kinds=None):
    kinds = CLSR_KINDS + SIB_KINDS + OWN_KINDS if kinds is None else tuple(kinds)
    out = clsr_sequences() if "clsr" in kinds else []
    out += sibling_sequences([k for k in kinds if k in SIB_KINDS])
    out += own_sequences([k for k in kinds if k in OWN_KINDS])
    return out


# ------------------------------------------------------------------------------------------ input conditions (feeds only)
def _mask(ids, V):
    m = torch.zeros(V, dtype=torch.bool)
    m[ids] = True
    return m


def table_rows(s, fam):
    return {name: int(s.dims["Vi" if "item" in key else ("Vc" if key == "cate" else "Vu")]) for key, name in fam.tmap.items()}


def input_conditions(s, fam=None):
    """Properties of the FEEDS, checked before anything runs: at every training step from the second on, the item table and
    every user table see at least one row that was never touched before and leave out at least one row that was (the
    12-row category table is exempt).  -> list of problems"""
    fam = fam or family(s.kind)
    V = table_rows(s, fam)
    keys = ("item",) + tuple(fam.user_tables)
    ever, problems, n = {}, [], 0
    for no, (what, shape, variant) in enumerate(SCHEDULE, 1):
        if what != "train":
            continue
        n += 1
        rows = fam.touched(get_feed(s, shape, variant))
        for key in keys:
            name = fam.tmap[key]
            now = _mask(rows[name], V[name])
            if n > 1:
                if not bool((now & ~ever[name]).any()):
                    problems.append("%s step %d: no row of %s is touched now and never before" % (s.id, no, key))
                if not bool((ever[name] & ~now).any()):
                    problems.append("%s step %d: no row of %s was touched before and is not touched now" % (s.id, no, key))
            ever[name] = now | ever.get(name, torch.zeros_like(now))
    return problems


def find_seeds(s, fam=None, tries=400):
    """``python scripts/fuzz_sequence.py seeds``: for every training step in order, the first feed seed (the default one, then
    default + 1000 k) with which the input conditions hold up to that step -- what SEEDS commits.  Feeds only, no oracle."""
    fam = fam or family(s.kind)
    found = {}
    for no, (what, shape, variant) in enumerate(SCHEDULE, 1):
        if what != "train":
            continue
        base = feed_seed(s, shape, variant)
        for k in range(tries):
            s.seeds[(shape, variant)] = base + 1000 * k
            s._feeds.pop((shape, variant), None)
            if not [p for p in input_conditions(s, fam) if " step %d:" % no in p]:
                break
        else:
            raise RuntimeError("%s step %d: no seed in %d tries" % (s.id, no, tries))
        if k:
            found[(shape, variant)] = base + 1000 * k
    return found


# ------------------------------------------------------------------------------------------ the two subjects
def _state(params, bn, m, v, clock):
    return types.SimpleNamespace(params=params, bn=bn, m=m, v=v, clock=clock)


class OracleSubject(object):
    """FUZZ_F32=cpu: the float32 oracle in the net's place.  Its state is float32, as a net's."""

    def __init__(self, s, fam, params32):
        self.s, self.fam = s, fam
        adam = O.init_adam(params32)
        self.st = _state(OrderedDict(params32), fam.init_bn(params32), {k: a[0] for k, a in adam.items()},
                         {k: a[1] for k, a in adam.items()}, 0.0)
        self.gradients = True

    def state(self):
        return self.st

    def train(self, shape, feed):
        st, fam = self.st, self.fam
        adam = OrderedDict((k, (st.m[k], st.v[k])) for k in st.m)
        new_p, new_bn, new_a, ls, grads, norms, out = fam.train(st.params, st.bn, adam, int(st.clock) + 1,
                                                                O.to_torch_feed(feed, dtype=torch.float32), self.s.hp, self.s.lazy,
                                                                group_of(self.s))
        f32 = lambda t: t.detach().float()
        self.st = _state(OrderedDict((k, f32(t)) for k, t in new_p.items()), OrderedDict((k, f32(t)) for k, t in new_bn.items()),
                         {k: f32(a[0]) for k, a in new_a.items()}, {k: f32(a[1]) for k, a in new_a.items()}, st.clock + 1)
        return dict(logit=out["logit"].detach(), model_output=out["model_output"].detach(),
                    losses={k: float(t) for k, t in ls.items()}, grads=out["raw_grads"], norms=norms, dense_norms=norms)

    def score(self, shape, feed):
        return self.fam.predict(self.st.params, self.st.bn, O.to_torch_feed(feed, dtype=torch.float32), self.s.hp)["logit"]

    def replayed(self):
        return None


class NetSubject(object):
    """The HIP net.  ``plans``: pass 1 (launch plans, one persistent uploaded feed object per shape); otherwise pass 2
    (no plans, gradients captured)."""

    def __init__(self, s, fam, params32, plans, precision):
        self.s, self.fam, self.plans = s, fam, plans
        self.net = net = fam.make_net(s.hp, s.dims, s.dedup, precision)
        sd = dict(params32)
        sd.update(fam.init_bn(params32))
        net.load_state_dict(sd, strict=True)        # the ONLY load: nothing is loaded between the steps
        net.use_plans, net.capture_grads = bool(plans), not plans
        self.gradients = not plans
        self.names = list(params32)
        self.up, self.calls = {}, {}

    def state(self):
        net, sd = self.net, self.net.state_dict()
        m, v = {}, {}
        for i, name in enumerate(net.dense_names):
            o, t = int(net.seg_off[i]), sd[name]
            m[name] = sd["__adam__/dense_m"][o:o + t.numel()].reshape(t.shape)
            v[name] = sd["__adam__/dense_v"][o:o + t.numel()].reshape(t.shape)
        for key, name in self.fam.tmap.items():
            m[name], v[name] = sd["__adam__/%s_m" % key], sd["__adam__/%s_v" % key]
        st = _state(OrderedDict((k, sd[k]) for k in self.names),
                    OrderedDict((k, t) for k, t in sd.items() if k.endswith(("/moving_mean", "/moving_variance"))),
                    m, v, float(sd["__adam__/state"][0]))
        st.raw = sd
        return st

    def _upload(self, shape, feed, training):
        if not self.plans:
            return self.net.upload(feed, training)
        f = self.up[shape] = self.net.upload(feed, training, into=self.up.get(shape))
        self.calls[id(f)] = self.calls.get(id(f), 0) + 1
        return f

    def train(self, shape, feed):
        net = self.net
        got = net.train_step(self._upload(shape, feed, True))
        torch.cuda.synchronize()
        res = dict(logit=got["logit"].detach().cpu().clone(), losses=net.read_losses(),
                   model_output=got["model_output"].detach().cpu().clone() if "model_output" in got else None)
        if self.gradients:
            cap = net.captured
            res["grads"] = {n: g.detach().cpu() for n, g in cap["dense"].items()}
            res["grads"].update({self.fam.tmap[k]: g.detach().cpu() for k, g in cap["tables"].items()})
            ss = cap["table_sumsq"].double().cpu().numpy()
            # (with de-duplicated histories too: the oracle then takes the norm of the group sums, group_of)
            res["norms"] = {self.fam.tmap[k]: float(sum(ss[i] for i in sl)) ** 0.5 for k, sl in self.fam.norm_slots.items()}
            ds = cap["dense_sumsq"].double().cpu().numpy()
            res["dense_norms"] = {n: float(ds[i]) ** 0.5 for i, n in enumerate(net.dense_names)}
        return res

    def score(self, shape, feed):
        got = self.net.forward(self._upload(shape, feed, False), False)
        torch.cuda.synchronize()
        return got["logit"].detach().cpu().clone()

    def replayed(self):
        """(training plans, scoring plans) recorded AND run a third time for the same feed object: replayed"""
        n = {"train": 0, "fwd": 0}
        for key, ent in self.net._step_plans.items():
            if len(ent) > 1 and ent[1] is not None and self.calls.get(key[1], 0) >= 3:
                n[key[0][0]] += 1
        return n["train"], n["fwd"]


# ------------------------------------------------------------------------------------------ the comparisons
def close_t(got, exp, rtol, atol, tag):
    """fuzz_step.close with a per-element absolute bar."""
    got, exp = got.double().reshape(-1), exp.double().reshape(-1)
    bar = (atol.double().reshape(-1) + rtol * exp.abs()).clamp_min(1e-300)
    err = (got - exp).abs()
    st = STATS.setdefault(tag, [0.0, 0.0, 0.0])
    if err.numel():
        st[:] = [max(st[0], float((err / bar).max())), max(st[1], float(err.max())), max(st[2], float(exp.abs().max()))]
    if not bool(torch.isfinite(got).all() and torch.isfinite(exp).all()):
        return "non-finite values: %d computed, %d expected" % (int((~torch.isfinite(got)).sum()), int((~torch.isfinite(exp)).sum()))
    if err.numel() and float((err - bar).max()) > 0:
        i = int((err / bar).argmax())
        return "max err / bar %.3f at element %d: got %.6e, expected %.6e" % (float((err / bar).max()), i, float(got[i]), float(exp[i]))
    return None


def _bits_equal(a, b):
    return a.float().contiguous().view(torch.int32) == b.float().contiguous().view(torch.int32)


def _rows_differ(a, b, rows):
    """ids among ``rows`` (bool [V]) at which the float32 tables a, b differ in any bit"""
    same = _bits_equal(a, b).reshape(a.shape[0], -1).all(1)
    return (rows & ~same).nonzero().reshape(-1)


def check_train(s, fam, pre, post, res, feed, ever, init, P):
    """One training step: the subject's outputs and post-step state against the float64 oracle stepped from ``pre``."""
    hp, lr = s.hp, float(s.hp.learning_rate)
    problems = []
    add = lambda what, e: problems.append("%s: %s" % (what, e)) if e else None
    dbl = lambda d: OrderedDict((k, t.double()) for k, t in d.items())
    params, bn = dbl(pre.params), dbl(pre.bn)
    adam = OrderedDict((k, (pre.m[k].double(), pre.v[k].double())) for k in pre.m)
    new_p, new_bn, new_a, ls, grads, norms, out = fam.train(params, bn, adam, int(pre.clock) + 1,
                                                            O.to_torch_feed(feed, dtype=torch.float64), hp, s.lazy, group_of(s))
    raw = out["raw_grads"]
    kind = s.kind
    # ---- values
    add("logit", close(res["logit"], out["logit"], 1e-4, 1e-4, ("logit", kind)))
    if res["model_output"] is None:
        problems.append("model_output: not returned by the step")
    else:
        add("model_output", close(res["model_output"], out["model_output"], 1e-4, 1e-5, ("model_output", kind)))
    for k in fam.loss_keys:
        add(k, close([res["losses"][k]], [float(ls[k])], 1e-5, 1e-7, ("loss", k)))
    # ---- the clock and the moving statistics
    if post.clock != pre.clock + 1:
        problems.append("Adam clock %r -> %r" % (pre.clock, post.clock))
    for k, t in new_bn.items():
        add(k, close(post.bn[k], t, 1e-4, 1e-6, ("bn", kind)))
    if set(post.bn) != set(pre.bn) or set(new_bn) - set(post.bn):
        problems.append("moving statistics: %d before, %d after, %d in the oracle" % (len(pre.bn), len(post.bn), len(new_bn)))
    tnames = {name: key for key, name in fam.tmap.items()}
    dense = [n for n in raw if n not in tnames]
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in dense)
    comparable = P > 1 or fam.p1_comparable
    if comparable:
        # ---- the tables: gradient and clip norm (pass 2 / float32 oracle) and the applied update, fuzz_step's own checks
        captured = "grads" in res
        problems += FS.table_checks("", fam.tmap, {k: res["grads"][n] for k, n in fam.tmap.items()} if captured else None,
                                    {k: res["norms"][n] for k, n in fam.tmap.items()} if captured else None,
                                    post.params, pre.params, (params, new_p, grads, raw, norms), floor, hp)
        for name in raw:
            tag = tnames.get(name, "dense")
            g = grads[name].double()
            scale = float(raw[name].abs().max()) + 1e-12
            c = O._clip_factor(norms[name] ** 2, float(hp.max_grad_norm)) if hp.is_clip_norm else 1.0
            a = c * (2e-4 * scale + floor)
            if name not in tnames:
                # ---- the dense variables: gradient and norm (pass 2 / float32 oracle), the update above noise level
                if captured:
                    add("grad " + name, close(res["grads"][name], raw[name], 2e-3, 2e-4 * scale + floor, ("grad", tag)))
                    add("norm " + name, close([res["dense_norms"][name]], [norms[name]], 1e-3, 20 * floor, ("norm", tag)))
                sel = g.reshape(-1).abs() > 100 * floor
                if int(sel.sum()):
                    add("adam update " + name, close((post.params[name].double() - params[name]).reshape(-1)[sel],
                                                     (new_p[name] - params[name]).reshape(-1)[sel], 5e-3, 0.02 * lr, ("update", tag)))
            # ---- the moments: their increments are linear / quadratic in g (the gradient bar, scaled; for v the rounding
            #      of the stored float32 moment on top, V_ROUND)
            m0, v0 = adam[name]
            m1, v1 = new_a[name]
            add("adam m " + name, close_t(post.m[name].double() - BETA1 * m0, m1 - BETA1 * m0, 0.0,
                                          (1 - BETA1) * (2e-3 * g.abs() + a), ("slot m", tag)))
            add("adam v " + name, close_t(post.v[name].double() - BETA2 * v0, v1 - BETA2 * v0, 0.0,
                                          (1 - BETA2) * (4e-3 * g * g + 2 * g.abs() * a + a * a) + V_ROUND * v1.abs(), ("slot v", tag)))
    # ---- table rows by history: never touched / touched earlier and not now
    rows = fam.touched(feed)
    for key, name in fam.tmap.items():
        V = params[name].shape[0]
        now = _mask(rows[name], V)
        before = ever.get(name, torch.zeros(V, dtype=torch.bool))
        ever[name] = before | now
        never, stale = ~ever[name], before & ~now
        STATS.setdefault(("never rows", key), [0.0, 0.0, 0.0])[2] += float(never.sum())
        STATS.setdefault(("stale rows", key), [0.0, 0.0, 0.0])[2] += float(stale.sum())
        for what, a_, b_ in (("rows", post.params[name], init.params[name]), ("m", post.m[name], init.m[name]),
                             ("v", post.v[name], init.v[name])):
            bad = _rows_differ(a_, b_, never)
            if len(bad):
                problems.append("%s %s: %d of %d never-touched rows differ from the loaded state, first %s" % (
                    name, what, len(bad), int(never.sum()), bad[:6].tolist()))
        if not int(stale.sum()):
            continue
        if s.lazy:
            for what, a_, b_ in (("rows", post.params[name], pre.params[name]), ("m", post.m[name], pre.m[name]),
                                 ("v", post.v[name], pre.v[name])):
                bad = _rows_differ(a_, b_, stale)
                if len(bad):
                    problems.append("lazyadam %s %s: %d of %d rows touched earlier and not now changed, first %s" % (
                        name, what, len(bad), int(stale.sum()), bad[:6].tolist()))
        else:
            # dense Adam keeps decaying the moments of such a row and keeps moving it
            upd_got = (post.params[name].double() - params[name])[stale]
            add("adam decay of rows not touched now, " + name,
                close(upd_got, (new_p[name] - params[name])[stale], 5e-3, 0.02 * lr, ("stale update", key)))
            if not comparable:      # (the moments of these rows: their gradient is exactly zero on both sides)
                for what, got_, exp_ in (("m", post.m[name], new_a[name][0]), ("v", post.v[name], new_a[name][1])):
                    add("adam decay %s %s" % (what, name), close_t(got_[stale], exp_[stale], 0.0, DECAY_ROUND * exp_[stale].abs(),
                                                                    ("stale slot " + what, key)))
            if key.startswith("item") and not float(upd_got.abs().max()) > 0.02 * lr:
                problems.append("adam %s: no row touched earlier and not now moved by more than 0.02 lr (largest %.3e)" % (
                    name, float(upd_got.abs().max())))
    for name in pre.params:           # tables the model never trains (user_embedding)
        if name not in raw and not bool(_bits_equal(post.params[name], pre.params[name]).all()):
            problems.append("untrained variable %s changed" % name)
    return problems


def states_identical(a, b):
    bad = []
    da, db = getattr(a, "raw", None), getattr(b, "raw", None)
    if da is None:
        da = dict(a.params, **a.bn)
        da.update({"m/" + k: t for k, t in a.m.items()})
        da.update({"v/" + k: t for k, t in a.v.items()})
        db = dict(b.params, **b.bn)
        db.update({"m/" + k: t for k, t in b.m.items()})
        db.update({"v/" + k: t for k, t in b.v.items()})
        da["clock"], db["clock"] = torch.tensor([a.clock]), torch.tensor([b.clock])
    if set(da) != set(db):
        return ["state keys differ"]
    for k in da:
        x, y = torch.as_tensor(da[k]), torch.as_tensor(db[k])
        if x.shape != y.shape or not torch.equal(x, y):
            bad.append(k)
    return bad


def run_pass(s, fam, subject, label):
    """The schedule on one subject.  -> list of problems, each with the step number."""
    problems = []
    init = subject.state()
    ever = {}
    for no, (what, shape, variant) in enumerate(SCHEDULE, 1):
        feed = get_feed(s, shape, variant)
        pre = subject.state()
        here = []
        if what == "train":
            res = subject.train(shape, feed)
            here = check_train(s, fam, pre, subject.state(), res, feed, ever, init, s.shapes[shape]["P"])
        else:
            dbl = lambda d: OrderedDict((k, t.double()) for k, t in d.items())
            exp = fam.predict(dbl(pre.params), dbl(pre.bn), O.to_torch_feed(feed, dtype=torch.float64), s.hp)["logit"]
            for rep in (1, 2):      # twice: the second scoring of the schedule then REPLAYS the plan the first recorded
                e = close(subject.score(shape, feed), exp, 1e-4, 1e-4, ("eval logit", s.kind))
                if e:
                    here.append("eval logit (forward %d): %s" % (rep, e))
            bad = states_identical(pre, subject.state())
            if bad:
                here.append("scoring changed the state: %s" % bad[:6])
        problems += ["%s step %d (%s %s): %s" % (label, no, what, shape, p) for p in here]
    rp = subject.replayed()
    if rp is not None and label.startswith("pass 1") and (rp[0] < 1 or rp[1] < 1):
        problems.append("%s: %d training and %d scoring plans were replayed, at least one of each expected" % ((label,) + rp))
    return problems


def run_sequence(s, precision="fp32", cpu=None):
    """Every pass of one committed sequence.  -> list of problems"""
    cpu = os.environ.get("FUZZ_F32") == "cpu" if cpu is None else cpu
    fam = family(s.kind)
    problems = input_conditions(s, fam)
    if problems:
        return problems
    params32 = fam.init_params(s.dims, s.hp, s.param_seed)
    if cpu:
        return run_pass(s, fam, OracleSubject(s, fam, params32), "float32 oracle")
    for plans in (True, False):
        subject = NetSubject(s, fam, params32, plans, precision)
        problems += run_pass(s, fam, subject, "pass %d" % (1 if plans else 2))
    return problems


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "seeds":
        for s in sequences():
            s.seeds.clear()
            print("    %r: %r," % (s.id, find_seeds(s)))
        return
    kinds = sys.argv[1].split(",") if len(sys.argv) > 1 else None
    precision = os.environ.get("FUZZ_PRECISION", "fp32")
    bad = n = 0
    merged = {}
    for s in sequences(kinds):
        n += 1
        STATS.clear()
        try:
            problems = run_sequence(s, precision)
        except Exception:
            bad += 1
            print("CRASH " + s.desc)
            print("    " + traceback.format_exc().strip().splitlines()[-1][:400])
            if os.environ.get("FUZZ_TRACE"):
                traceback.print_exc()
            if os.environ.get("FUZZ_F32") != "cpu":
                torch.cuda.synchronize()      # a device fault ends the run here: nothing more is started on that GPU
            continue
        for tag, st in STATS.items():
            m = merged.setdefault(tag, [0.0, 0.0, 0.0])
            m[:] = [max(m[0], st[0]), max(m[1], st[1]), m[2] + st[2] if tag[0].endswith(" rows") else max(m[2], st[2])]
        if problems:
            bad += 1
            print("FAIL " + s.desc)
            for p in problems[:12]:
                print("    " + p)
        else:
            print("ok   %-22s worst err / bar %.3f" % (s.id, FS.worst_ratio()))
    print("%d of %d sequences with problems" % (bad, n))
    STATS.clear()
    STATS.update(merged)
    by_check = {}
    for tag, st in STATS.items():
        by_check[tag[0]] = max(by_check.get(tag[0], 0.0), st[0])
    FS.print_stats()
    print("    worst ratio per bar: " + ", ".join("%s %.3f" % kv for kv in sorted(by_check.items()) if not kv[0].endswith(" rows")))


if __name__ == "__main__":
    main()
