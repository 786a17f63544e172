"""GPU tests of bf16 embedding tables with an exact fp32 master (``CLSRNet(table_dtype="bf16", table_master=True)``;
include/clsr_hip.h: the ``_hm`` kernels).  The table is the pair (hi = the bf16 values every lookup reads, lo = a 16-bit
residual) with  bits(master) = (hi << 16) + sign_extend(lo)  mod 2^32,  hi = (bits + 0x8000) >> 16.

Every `_hm` kernel inlines the element update of the fp32 kernel on the same launch path (csrc/tableopt.h: adam_elem): its
moments equal the fp32 kernel's and merge(hi, lo) equals the fp32 table, bit for bit.  Where a whole step is compared
with the fp32 net (other gradients' norms come from float64 atomics) the bar is  1e-6 |w| + 1e-6 U  (U: the largest
|delta w| of the case)."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

from clsr_amd import ops  # noqa: E402
from clsr_amd.ops import call  # noqa: E402
# (shared with the random-shape differential of the table modes, tests/test_fuzz_tables_gpu.py)
from fuzz_tables import BF, DEV, I16, bits16, merge, split  # noqa: E402
from fuzz_tables import master_bar as _master_bar  # noqa: E402


# ------------------------------------------------------------------------------------------- the encoding, restated
def np_split(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    hi = ((b + 0x8000) & 0xFFFFFFFF) >> 16
    lo = (b - (hi << 16)) & 0xFFFF
    nonfinite = (b & 0x7F800000) == 0x7F800000
    hi = np.where(nonfinite, (b >> 16) | np.where((b & 0x007FFFFF) != 0, 0x0040, 0), hi)
    lo = np.where(nonfinite, 0, lo)
    return hi.astype(np.uint16), lo.astype(np.uint16).view(np.int16)


def np_merge(hi, lo):
    b = ((hi.astype(np.int64) << 16) + lo.astype(np.int64)) & 0xFFFFFFFF
    return b.astype(np.uint32).view(np.float32)


def test_split_and_merge_against_the_restatement():
    g = torch.Generator().manual_seed(11)
    hand = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x80008000, 0x00018000, 0x00000000,
                     0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF,
                     0x7F7F8000, 0x3F800000, 0x3F7FFFFF, 0x3F807FFF, 0x3F808001, 0x7F800000, 0xFF800000, 0x7FC00000,
                     0x7F800001, 0xFFFFFFFF, 0xFFFF8000, 0x7F808000, 0xFFC00001], dtype=np.uint32).view(np.float32)
    for n in (37 * 8, 300 * 32, 5000 * 96 + 3):
        rnd = (torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 60 - 40)).numpy()
        x = np.concatenate([hand, rnd.astype(np.float32), np.random.RandomState(n).randint(
            0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)])
        xd = torch.from_numpy(x).to(DEV)
        hi, lo = split(xd)
        back = merge(hi, lo)
        torch.cuda.synchronize()
        hi_n, lo_n = bits16(hi).cpu().numpy().view(np.uint16), lo.cpu().numpy()
        eh, el = np_split(x)
        assert np.array_equal(hi_n, eh) and np.array_equal(lo_n, el), "hi / lo == the restatement, bit for bit"
        fin = np.isfinite(x)
        b_in, b_out = x.view(np.uint32), back.cpu().numpy().view(np.uint32)
        assert np.array_equal(b_out[fin], b_in[fin]), "merge(split(x)) == x for every finite x"
        assert np.array_equal(b_out, np_merge(eh, el).view(np.uint32))
        wide = hi.float().cpu().numpy()
        assert not np.isfinite(wide[~fin]).any() and not np.isfinite(back.cpu().numpy()[~fin]).any()
        assert np.array_equal(np.isnan(wide[~fin]), np.isnan(x[~fin])), "inf stays inf, NaN stays NaN"
        # half a bf16 ulp: 2^15 fp32 spacings of x (where bf16 itself does not overflow: |x| < 0x7f7f8000)
        ok = fin & np.isfinite(wide)
        assert np.array_equal(ok, fin & (np.abs(x) < np.array([0x7F7F8000], dtype=np.uint32).view(np.float32)[0]))
        half = np.spacing(np.abs(x[ok])).astype(np.float64) * 2.0 ** 15
        assert bool((np.abs(x[ok].astype(np.float64) - wide[ok].astype(np.float64)) <= half).all())
        ties = (b_in & 0xFFFF) == 0x8000
        keep = torch.from_numpy(fin & ~ties).to(DEV)
        assert torch.equal(bits16(xd.to(BF))[keep], bits16(hi)[keep]), "hi == the nearest-even bf16 except at exact ties"


# ------------------------------------------------------------------------------------------- kernel level
SHAPES = [(37, 8, 5), (300, 32, 300), (5000, 96, 777)]


def _case(V, C, nrows, seed=None, abort=0.0):
    """Inputs and Adam state of test_lazy_adam_rows_on_a_bf16_table, with a master that is NOT bf16-representable."""
    g = torch.Generator().manual_seed(V if seed is None else seed)
    w = (torch.randn(V, C, generator=g) * 0.05).to(DEV)
    ids = torch.randperm(V, generator=g)[:nrows].sort()[0].int().to(DEV)
    grad = torch.zeros(V, C, device=DEV)
    grad[ids.long()] = torch.randn(nrows, C, generator=g).to(DEV) * 1e-2
    m0, v0 = torch.randn(V, C, generator=g).to(DEV) * 1e-3, torch.rand(V, C, generator=g).to(DEV) * 1e-5
    flags = torch.zeros(V, dtype=torch.uint8, device=DEV)
    flags[ids.long()] = 1
    sumsq = torch.tensor([float((grad.double() ** 2).sum())], dtype=torch.float64, device=DEV)
    state = torch.tensor([3.0, 0.9 ** 3, 0.999 ** 3, 1e-3 * (1 - 0.999 ** 3) ** 0.5 / (1 - 0.9 ** 3), abort],
                         dtype=torch.float64, device=DEV)
    return dict(w=w, ids=ids, count=torch.tensor([nrows], dtype=torch.int32, device=DEV), grad=grad, m=m0, v=v0,
                flags=flags, sumsq=sumsq, state=state, V=V, C=C, nrows=nrows)


def _check_update(c, hi, lo, gr, m, v, fl, tf, gf, mf, vf, ff, touched, name):
    hi0, lo0 = split(c["w"])
    h2, l2 = split(merge(hi, lo))
    assert torch.equal(bits16(h2), bits16(hi)) and torch.equal(l2, lo), "the stored (hi, lo) is canonical"
    untouched = ~touched
    assert torch.equal(bits16(hi)[untouched], bits16(hi0)[untouched]) and torch.equal(lo[untouched], lo0[untouched])
    assert torch.equal(gr, gf) and torch.equal(fl, ff), "gradient rows and flags cleared as by the fp32 kernel"
    assert float(gr[touched].abs().max()) == 0.0
    assert torch.equal(m, mf) and torch.equal(v, vf), name + ": the moments of the fp32 kernel"
    assert torch.equal(merge(hi, lo), tf), name + ": the master is the fp32 kernel's table"
    assert not torch.equal(tf[touched], c["w"][touched])


@pytest.mark.parametrize("V,C,nrows", SHAPES)
def test_row_update_with_master(V, C, nrows):
    c = _case(V, C, nrows)
    hi, lo = split(c["w"])
    assert torch.equal(merge(hi, lo), c["w"])
    gr, m, v, fl = c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()
    call("clsr_table_adam_rows_hm", hi, lo, gr, m, v, fl, c["ids"], c["count"], nrows, C, c["sumsq"], 1, 1, 2.0, c["state"],
         0.9, 0.999, 1e-8)
    tf, gf, mf, vf, ff = c["w"].clone(), c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()
    call("clsr_table_adam_rows", tf, gf, mf, vf, ff, c["ids"], c["count"], nrows, C, c["sumsq"], 1, 1, 2.0, c["state"],
         0.9, 0.999, 1e-8)
    torch.cuda.synchronize()
    touched = torch.zeros(V, dtype=torch.bool, device=DEV)
    touched[c["ids"].long()] = True
    _check_update(c, hi, lo, gr, m, v, fl, tf, gf, mf, vf, ff, touched, "rows_hm %r" % ((V, C, nrows),))
    assert int(fl.sum()) == 0


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("V,C,nrows", SHAPES)
def test_single_table_sweep_with_master(V, C, nrows, lazy):
    c = _case(V, C, nrows)
    hi, lo = split(c["w"])
    gr, m, v, fl = c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()
    call("clsr_table_adam_hm", hi, lo, gr, m, v, fl, V, C, c["sumsq"], 1, 1, 2.0, c["state"], 0.9, 0.999, 1e-8, lazy)
    tf, gf, mf, vf, ff = c["w"].clone(), c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()
    call("clsr_table_adam", tf, gf, mf, vf, ff, V, C, c["sumsq"], 1, 1, 2.0, c["state"], 0.9, 0.999, 1e-8, lazy)
    torch.cuda.synchronize()
    touched = c["flags"].bool() if lazy else torch.ones(V, dtype=torch.bool, device=DEV)
    _check_update(c, hi, lo, gr, m, v, fl, tf, gf, mf, vf, ff, touched, "table_adam_hm lazy=%d %r" % (lazy, (V, C)))
    assert int(fl.sum()) == 0


def _desc_row(table, c, gr, m, v, fl):
    # clsr_table_desc: table, partner, grad, m, v, flags, sumsq_reg, disc_loss, sumsq_adam, V, C, nsum, sumsq_stride, ...
    return (table.data_ptr(), None, gr.data_ptr(), m.data_ptr(), v.data_ptr(), fl.data_ptr(), None, None,
            c["sumsq"].data_ptr(), c["V"], c["C"], 1, 1, 0.0, 0.0, 0)


# two tables per launch; C = 6 puts the launch on the scalar form (the other cases: 16-byte form)
@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("shapes", [((37, 8, 5), (300, 32, 300)), ((5000, 96, 777), (37, 8, 5)), ((37, 6, 5), (300, 32, 300))])
def test_multi_table_sweep_with_master(shapes, lazy):
    cs = [_case(*s, seed=100 + i) for i, s in enumerate(shapes)]
    st = cs[0]["state"]
    got, ref = [], []
    for c in cs:
        hi, lo = split(c["w"])
        got.append((hi, lo, c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()))
        ref.append((c["w"].clone(), c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()))
    ops.multi("clsr_tables_adam_multi_hm", ops.TableDesc,
              [_desc_row(t[0], c, t[2], t[3], t[4], t[5]) for t, c in zip(got, cs)], 2.0, st, 0.9, 0.999, 1e-8, lazy,
              lo=[t[1].data_ptr() for t in got])
    ops.multi("clsr_tables_adam_multi", ops.TableDesc,
              [_desc_row(t[0], c, t[1], t[2], t[3], t[4]) for t, c in zip(ref, cs)], 2.0, st, 0.9, 0.999, 1e-8, lazy)
    torch.cuda.synchronize()
    for c, (hi, lo, gr, m, v, fl), (tf, gf, mf, vf, ff) in zip(cs, got, ref):
        touched = c["flags"].bool() if lazy else torch.ones(c["V"], dtype=torch.bool, device=DEV)
        _check_update(c, hi, lo, gr, m, v, fl, tf, gf, mf, vf, ff, touched,
                      "tables_adam_multi_hm lazy=%d %r" % (lazy, (c["V"], c["C"])))
        assert int(fl.sum()) == 0


@pytest.mark.parametrize("V,C,nrows", [(37, 8, 5), (300, 32, 300), (37, 6, 5)])
def test_aborted_step_touches_nothing(V, C, nrows):
    c = _case(V, C, nrows, abort=1.0)
    hi0, lo0 = split(c["w"])

    def fresh():
        return hi0.clone(), lo0.clone(), c["grad"].clone(), c["m"].clone(), c["v"].clone(), c["flags"].clone()

    runs = []
    if C % 4 == 0:
        t = fresh()
        call("clsr_table_adam_rows_hm", t[0], t[1], t[2], t[3], t[4], t[5], c["ids"], c["count"], nrows, C, c["sumsq"], 1, 1,
             2.0, c["state"], 0.9, 0.999, 1e-8)
        runs.append(t)
    for lazy in (0, 1):
        t = fresh()
        call("clsr_table_adam_hm", t[0], t[1], t[2], t[3], t[4], t[5], V, C, c["sumsq"], 1, 1, 2.0, c["state"], 0.9, 0.999,
             1e-8, lazy)
        runs.append(t)
        t = fresh()
        ops.multi("clsr_tables_adam_multi_hm", ops.TableDesc, [_desc_row(t[0], c, t[2], t[3], t[4], t[5])], 2.0, c["state"],
                  0.9, 0.999, 1e-8, lazy, lo=[t[1].data_ptr()])
        runs.append(t)
    torch.cuda.synchronize()
    for hi, lo, gr, m, v, _ in runs:
        assert torch.equal(bits16(hi), bits16(hi0)) and torch.equal(lo, lo0)
        assert torch.equal(gr, c["grad"]) and torch.equal(m, c["m"]) and torch.equal(v, c["v"])


def test_small_updates_survive_with_the_master():
    """A table of 1.0 under a constant gradient, 16 lazy-Adam steps at lr 1e-3: the plain bf16 table never moves (1 - 0.001
    rounds back to 1.0, the parent's behaviour), the master follows the fp32 trajectory and its bf16 half ends below 1.0."""
    V, C, nrows = 37, 8, 5
    ids = torch.tensor([0, 7, 8, 20, 36], dtype=torch.int32, device=DEV)
    count = torch.tensor([nrows], dtype=torch.int32, device=DEV)
    g0 = torch.zeros(V, C, device=DEV)
    g0[ids.long()] = 0.01
    f0 = torch.zeros(V, dtype=torch.uint8, device=DEV)
    f0[ids.long()] = 1
    sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
    one = torch.ones(V, C, device=DEV)
    runs = {}
    for kind in ("h", "hm", "f"):
        state = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
        m, v = torch.zeros(V, C, device=DEV), torch.zeros(V, C, device=DEV)
        tab = {"h": (one.to(BF),), "hm": split(one), "f": (one.clone(),)}[kind]
        traj = []
        for _ in range(16):
            call("clsr_adam_tick", state, 1e-3, 0.9, 0.999)
            call({"h": "clsr_table_adam_rows_h", "hm": "clsr_table_adam_rows_hm", "f": "clsr_table_adam_rows"}[kind], *tab,
                 g0.clone(), m, v, f0.clone(), ids, count, nrows, C, sumsq, 1, 1, 0.0, state, 0.9, 0.999, 1e-8)
            traj.append(merge(*tab) if kind == "hm" else tab[0].float().clone())
        runs[kind] = (tab, traj)
    torch.cuda.synchronize()
    assert torch.equal(runs["h"][0][0].float(), one), "without a master every element is still exactly 1.0"
    prev = one
    for s, (a, b) in enumerate(zip(runs["hm"][1], runs["f"][1])):
        _master_bar(a, b, prev, "step %d" % (s + 1))
        prev = b
    hi = runs["hm"][0][0].float()
    assert bool((hi[ids.long()] < 1.0).all()) and torch.equal(hi[(f0 == 0)], one[(f0 == 0)])
    assert abs(float(runs["hm"][1][-1][0, 0]) - (1.0 - 16e-3)) < 1e-4      # Adam under a constant gradient: lr per step


# ------------------------------------------------------------------------------------------- net level
def _setup(golden_dir, golden_hparams, lazy=False, representable=True, optimizer=None):
    from clsr_amd.params import TABLES
    from oracle import clsr_oracle as O

    hp = copy.deepcopy(golden_hparams)
    hp.item_embedding_dim, hp.cate_embedding_dim = 32, 8
    if lazy:
        hp.optimizer = "lazyadam"
    if optimizer:
        hp.optimizer = optimizer
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    gf = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feeds = [{k[3:]: gf[k] for k in gf.files if k.startswith("b%d_" % b)} for b in range(2)]
    params = O.init_params(dims, hp, seed=3, scale_dense=8.0)
    if representable:
        for name in TABLES.values():
            params[name] = params[name].to(BF).float()
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    return hp, dims, feeds, sd, TABLES


@pytest.mark.parametrize("lazy", [False, True])
def test_step_with_master_tables(golden_dir, golden_hparams, lazy):
    """One train step on bf16 + master (sweep launches and row-list launches), plain bf16 and fp32 nets that hold the same
    bf16-representable tables: identical forward and gradients; the master follows the fp32 net, its bf16 half is the
    master's rounding."""
    from clsr_amd.net import CLSRNet

    hp, dims, feeds, sd, TABLES = _setup(golden_dir, golden_hparams, lazy=lazy)
    res = {}
    for tag, kw, rowlist in (("master", dict(table_dtype="bf16", table_master=True), False),
                             ("master_rows", dict(table_dtype="bf16", table_master=True), True),
                             ("bf16", dict(table_dtype="bf16"), False), ("fp32", dict(), False)):
        net = CLSRNet(hp, dims, device="cuda:0", seed=0, **kw)
        if rowlist:
            net.rowlist_min_elems = 0       # every table through the row-list (lazy) / single-table (dense) entries
        net.load_state_dict(copy.deepcopy(sd))
        net.capture_grads = True
        out = net.train_step(net.upload(feeds[1], True))
        torch.cuda.synchronize()
        res[tag] = (net, out["logit"].clone(), net.read_losses(), {k: v.clone() for k, v in net.captured["tables"].items()})
    nf = res["fp32"][0]
    for tag in ("master", "master_rows", "bf16"):
        assert torch.equal(res[tag][1], res["fp32"][1]), "%s: same looked-up values -> identical logits" % tag
        for k, v in res[tag][3].items():
            assert torch.equal(v, res["fp32"][3][k]), "%s: gradient table %s" % (tag, k)
        for k, v in res[tag][2].items():
            # (every loss term is a float64 sum that workgroups add with atomics in no fixed order: two runs of ONE net already
            #  differ in its last bits, so `==` cannot be asserted.  The bf16 nets run the same `_h` kernels on the same bits:
            #  only that reordering, a few thousand partial sums at 2^-53 each -> 1e-12; the fp32 net runs another
            #  instantiation: the bar of test_step_with_bf16_tables)
            print("%s %s: %.17g (bf16 %.17g, fp32 %.17g)" % (tag, k, v, res["bf16"][2][k], res["fp32"][2][k]))
            assert abs(v - res["fp32"][2][k]) <= 1e-9 * max(1.0, abs(res["fp32"][2][k])), (tag, k)
            assert abs(v - res["bf16"][2][k]) <= 1e-12 * max(1.0, abs(res["bf16"][2][k])), (tag, k)
    for tag in ("master", "master_rows"):
        nm = res[tag][0]
        assert set(nm.tab_lo) == set(nm.tables)
        for k in nm.tables:
            assert nm.tables[k].dtype == BF and nm.tab_lo[k].dtype == I16 and nm.tab_lo[k].shape == nm.tables[k].shape
            assert nm.P[TABLES[k]] is nm.tables[k]
            mk = nm.master(k)
            _master_bar(mk, nf.tables[k], torch.as_tensor(sd[TABLES[k]]), "%s %s" % (tag, k))
            h, l = split(mk)
            assert torch.equal(bits16(h), bits16(nm.tables[k])) and torch.equal(l, nm.tab_lo[k])
            assert not torch.equal(nf.tables[k].cpu(), torch.as_tensor(sd[TABLES[k]]))
    # sweep launches against row-list / single-table launches: both update (and clear) the same rows
    a, b = res["master"][0], res["master_rows"][0]
    for k in a.tables:
        d = (a.master(k).double() - b.master(k).double()).abs().max()
        print("default path vs row-list path, %s: max |diff| %.3e" % (k, float(d)))
        assert torch.equal(bits16(a.tables[k]), bits16(b.tables[k])) and torch.equal(a.tab_lo[k], b.tab_lo[k]), k


def test_master_checkpoints(golden_dir, golden_hparams):
    from clsr_amd.net import CLSRNet

    hp, dims, feeds, sd, TABLES = _setup(golden_dir, golden_hparams, representable=False)
    mk = lambda seed, **kw: CLSRNet(hp, dims, device="cuda:0", seed=seed, table_dtype="bf16", **kw)  # noqa: E731
    a = mk(0, table_master=True)
    # construction: the master is what this seed draws for an fp32 net
    f = CLSRNet(hp, dims, device="cuda:0", seed=0)
    for k in a.tables:
        assert torch.equal(a.master(k), f.tables[k]), k
    a.load_state_dict(copy.deepcopy(sd))
    plain = mk(0)
    plain.load_state_dict(copy.deepcopy(sd))
    out, out_plain = a.state_dict(), plain.state_dict()
    lost = 0.0
    for k, name in TABLES.items():
        src = torch.as_tensor(np.asarray(sd[name]), dtype=torch.float32)
        assert out[name].dtype == torch.float32 and torch.equal(out[name].view(torch.int32), src.view(torch.int32)), name
        lost += float((out_plain[name] - src).abs().sum())
    assert lost > 0.0, "a bf16 table without a master cannot return these values"
    assert set(out) == set(out_plain)
    # conversions in row chunks (what tables above master_chunk_elems elements get) give the same bits
    a.master_chunk_elems = 1000
    out_chunked = a.state_dict()
    b = mk(1, table_master=True)
    b.master_chunk_elems = 777
    b.load_state_dict(out_chunked)
    for k, name in TABLES.items():
        assert torch.equal(out_chunked[name], out[name])
        assert torch.equal(bits16(a.tables[k]), bits16(b.tables[k])) and torch.equal(a.tab_lo[k], b.tab_lo[k]), k
    for net in (a, b):
        net.train_step(net.upload(feeds[0], True))
    torch.cuda.synchronize()
    moved = 0
    for k, name in TABLES.items():
        assert torch.equal(bits16(a.tables[k]), bits16(b.tables[k])) and torch.equal(a.tab_lo[k], b.tab_lo[k]), k
        assert torch.equal(a.tab_m[k], b.tab_m[k]) and torch.equal(a.tab_v[k], b.tab_v[k]), k
        moved += int((a.master(k).cpu() != out[name]).sum())
    assert moved > 0


def test_master_arguments(golden_hparams):
    from clsr_amd.clsr import CLSRModel, GRU4RecModel
    from clsr_amd.net import CLSRNet
    from clsr_amd.seqnet import SeqNet
    from clsr_amd.sequential_iterator import SASequentialIterator

    hp = copy.deepcopy(golden_hparams)
    hp.item_embedding_dim, hp.cate_embedding_dim = 32, 8
    dims = dict(Vu=50, Vi=60, Vc=7)
    with pytest.raises(ValueError):
        CLSRNet(hp, dims, device="cuda:0", table_dtype="fp32", table_master=True)
    hp2 = copy.deepcopy(hp)
    hp2.optimizer = "adagrad"
    with pytest.raises(NotImplementedError):
        CLSRNet(hp2, dims, device="cuda:0", table_dtype="bf16", table_master=True)
    with pytest.raises(NotImplementedError):
        SeqNet(hp, dims, kind="gru4rec", device="cuda:0", table_dtype="bf16", table_master=True)
    with pytest.raises(NotImplementedError):        # the model API: sibling models refuse, CLSRModel passes it through
        GRU4RecModel(hp, SASequentialIterator, table_master=True)
    with pytest.raises(NotImplementedError):
        GRU4RecModel(hp, SASequentialIterator, table_dtype="bf16", table_master=True)
    model = CLSRModel(hp, SASequentialIterator, seed=1, table_dtype="bf16", table_master=True)
    assert model.net.table_master and set(model.net.tab_lo) == set(model.net.tables)
    assert CLSRModel(hp, SASequentialIterator, seed=1, table_dtype="bf16").net.table_master is False
    assert CLSRNet(hp, dims, device="cuda:0", table_dtype="bf16").table_master is False
