#!/usr/bin/env python
"""Exact differential of the embedding-table modes of CLSRNet at random shapes (test infrastructure, like tests/).

Shapes and hyper-parameters come from the generator of scripts/fuzz_step.py, restricted to what bf16 tables accept
(item width a multiple of 8, category width 8, adam / lazyadam).  Five nets hold the same bf16-representable tables:

    fp32        fp32 tables                      fp32_rows    ... every table through the row-list optimizer entries
    bf16        table_dtype="bf16"
    master      bf16 + table_master=True         master_rows  ... through the row-list entries

Same looked-up values, everything behind the lookups deterministic: logits and gradient tables are identical bit for bit;
the fp32 master follows the fp32 net's update (master_bar), its bf16 half is its rounding, the row-list launches equal the
sweeps.  A second step on another, smaller batch starts from the state the master net reached -- residuals that are no
longer zero -- with the nets that have no master reloaded on the master's bf16 half, so that all five look up the same
values again.

    python scripts/fuzz_tables.py          # the cases of tests/test_fuzz_tables_gpu.py
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_step  # noqa: E402
from clsr_amd.ops import call  # noqa: E402
from clsr_amd.params import TABLES  # noqa: E402
from oracle import clsr_oracle as O  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
I16 = torch.int16

MODES = (("fp32", dict(), False), ("fp32_rows", dict(), True), ("bf16", dict(table_dtype="bf16"), False),
         ("master", dict(table_dtype="bf16", table_master=True), False),
         ("master_rows", dict(table_dtype="bf16", table_master=True), True))

# (pinned part of the case, seed of its random rest); at least: D = 16 / T = 1, D = 64 / T = 50 / lognormal lengths, D = 128,
# one positive only, groups of 10 rows, both optimizers
CASES = [
    (dict(D=16, Dc=8, T=1), 1),
    (dict(D=64, Dc=8, T=50, lengths="lognormal"), 2),
    (dict(D=128, Dc=8), 3),
    (dict(P=1), 4),
    (dict(G=10, optimizer="lazyadam"), 5),
    (dict(optimizer="adam"), 6),
    (dict(optimizer="lazyadam", is_clip_norm=1, max_grad_norm=0.01), 7),
    (dict(), 8),
]


# ------------------------------------------------------------------------------------------- the (hi, lo) encoding
def split(x):
    hi = torch.empty(x.shape, dtype=BF, device=DEV)
    lo = torch.empty(x.shape, dtype=I16, device=DEV)
    call("clsr_table_split_hm", x.contiguous(), hi, lo, x.numel())
    return hi, lo


def merge(hi, lo):
    out = torch.empty(hi.shape, dtype=torch.float32, device=DEV)
    call("clsr_table_merge_hm", hi, lo, out, hi.numel())
    return out


def bits16(t):
    return t.view(I16)


def master_bar(got, ref, before, name):
    """|got - ref| <= 1e-6 |ref| + 1e-6 U, U = the largest |ref - before| (prints the measured maximum first)."""
    got, ref, before = got.double().cpu(), ref.double().cpu(), before.double().cpu()
    U = float((ref - before).abs().max())
    err = (got - ref).abs()
    bar = 1e-6 * ref.abs() + 1e-6 * U
    print("%s: max |master - fp32| = %.3e, U = %.3e, worst err / bar = %.3f"
          % (name, float(err.max()), U, float((err / bar.clamp_min(1e-300)).max())))
    assert bool((err <= bar).all()), "%s: max err %.3e against U %.3e" % (name, float(err.max()), U)
    return U


# ------------------------------------------------------------------------------------------- cases
def accepts_bf16(c):
    return c.Dc == 8 and (c.D - c.Dc) % 8 == 0 and c.D % 4 == 0


def draw(pin, seed, idx=0):
    """A fuzz_step draw that bf16 tables accept (drawn again until it is one; a pinned D decides at once)."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        c = fuzz_step.draw_case(rng, idx, "clsr", pin=pin)
        if accepts_bf16(c):
            return c
    raise RuntimeError("no acceptable draw for %r" % (pin,))


def draw_rejected(seed):
    """A fuzz_step draw that bf16 tables do NOT accept (category width 4, or an item width that is no multiple of 8)."""
    rng = np.random.default_rng(seed)
    while True:
        c = fuzz_step.draw_case(rng, 0, "clsr")
        if not accepts_bf16(c):
            return c


def _same_tables(a, b, what):
    for k in a.tables:
        assert torch.equal(bits16(a.tables[k]), bits16(b.tables[k])) and torch.equal(a.tab_lo[k], b.tab_lo[k]), (what, k)


def _step(nets, feed, before, values_only, what):
    """One captured training step of the five nets on ``feed`` and the assertions between them.  ``before``: variable name ->
    the fp32 nets' table values before the step (device tensors); for the master nets the step starts from their own
    master, which reads the same bf16 values."""
    from clsr_amd.net import CLSRNet  # noqa: F401

    m_before = {tag: {k: nets[tag].master(k) for k in nets[tag].tables} for tag in ("master", "master_rows")}
    res = {}
    for tag, net in nets.items():
        net.capture_grads = True
        out = net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        res[tag] = (out["logit"].clone(), net.read_losses(), {k: v.clone() for k, v in net.captured["tables"].items()})
    for tag in nets:
        assert torch.equal(res[tag][0], res["fp32"][0]), "%s %s: same looked-up values -> identical logits" % (what, tag)
        assert bool(torch.isfinite(res[tag][0]).all())
        for k, v in res[tag][1].items():
            # (loss terms: float64 sums added with atomics in no fixed order; the bars of test_step_with_master_tables)
            assert abs(v - res["fp32"][1][k]) <= 1e-9 * max(1.0, abs(res["fp32"][1][k])), (what, tag, k)
            if tag in ("master", "master_rows"):
                assert abs(v - res["bf16"][1][k]) <= 1e-12 * max(1.0, abs(res["bf16"][1][k])), (what, tag, k)
    if values_only:     # one positive: every row identical, gradients decided by rounding noise on the ReLU kinks
        return
    for tag in nets:
        assert set(res[tag][2]) == set(TABLES)
        for k, v in res[tag][2].items():
            assert torch.equal(v, res["fp32"][2][k]), "%s %s: gradient table %s" % (what, tag, k)
    nf = nets["fp32"]
    moved = 0
    for tag in ("master", "master_rows"):
        nm = nets[tag]
        assert set(nm.tab_lo) == set(nm.tables)
        for k, name in TABLES.items():
            assert nm.tables[k].dtype == BF and nm.tab_lo[k].dtype == I16 and nm.tab_lo[k].shape == nm.tables[k].shape
            mk = nm.master(k)
            # the fp32 net moved  before -> nf.tables[k]; Adam's step does not depend on the weight it is applied to, so
            # the master moves by the same amount from ITS starting point (equal to `before` when the residuals are zero)
            ref = m_before[tag][k].double() + (nf.tables[k].double() - before[name].double())
            master_bar(mk, ref, m_before[tag][k], "%s %s %s" % (what, tag, k))
            h, l = split(mk)
            assert torch.equal(bits16(h), bits16(nm.tables[k])) and torch.equal(l, nm.tab_lo[k]), (what, tag, k)
            moved += int((nf.tables[k] != before[name]).sum())
    assert moved > 0
    _same_tables(nets["master"], nets["master_rows"], what + " sweep launches == row-list launches")
    # fp32: the row-list path against the sweep -- same gradient tables, one element update (csrc/tableopt.h): same bits
    a, b = nets["fp32"], nets["fp32_rows"]
    for k in res["fp32"][1]:
        assert abs(res["fp32"][1][k] - res["fp32_rows"][1][k]) <= 1e-6 * max(1.0, abs(res["fp32"][1][k])), (what, k)
    for k in a.tables:
        assert torch.equal(b.tables[k], a.tables[k]), "%s fp32 row-list path vs sweep, %s" % (what, k)
    for net in nets.values():       # every path leaves the flags and the gradient tables cleared for the next step
        for k in net.tables:
            assert int(net.tab_flags[k].sum()) == 0 and float(net.tab_grad[k].abs().max()) == 0.0, (what, k)


def one_case(pin, seed, idx=0):
    from clsr_amd.net import CLSRNet

    c = draw(pin, seed, idx)
    print(c.desc.split(" {")[0], c.hp.optimizer, flush=True)
    params = O.init_params(c.dims, c.hp, seed=seed, scale_dense=8.0)
    for name in TABLES.values():                      # bf16-representable table values
        params[name] = params[name].to(BF).float()
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    nets = {}
    for tag, kw, rowlist in MODES:
        net = CLSRNet(c.hp, c.dims, device="cuda:0", seed=0, **kw)
        if rowlist:
            net.rowlist_min_elems = 0       # every table through the row-list (lazy) / single-table (dense) entries
        net.load_state_dict(copy.deepcopy(sd))
        nets[tag] = net
    for k, name in TABLES.items():
        assert nets["bf16"].tables[k].dtype == BF and nets["fp32"].tables[k].dtype == torch.float32
        assert torch.equal(nets["master"].master(k).cpu(), params[name]) and int(nets["master"].tab_lo[k].abs().max()) == 0
    values_only = c.P == 1
    _step(nets, fuzz_step.make_feed(c), {n: params[n].to(DEV) for n in TABLES.values()}, values_only, "step 1")
    if values_only:
        return c
    # ---- second step: another, smaller batch, from the state the master net reached (non-zero residuals).  The nets
    # without a master are reloaded on the bf16 half of that state, the row-list master net on the state itself: all five
    # look up the same values and hold the same dense variables, BN statistics and Adam slots again
    nm = nets["master"]
    s1 = nm.state_dict()
    residuals = sum(int((nm.tab_lo[k] != 0).sum()) for k in nm.tables)
    assert residuals > 0, "the second step is to start from residuals that are not zero"
    s1_hi = dict(s1)
    for k, name in TABLES.items():
        assert torch.equal(s1[name], nm.master(k).cpu())
        s1_hi[name] = nm.tables[k].float().cpu()
    for tag in ("fp32", "fp32_rows", "bf16"):
        nets[tag].load_state_dict(copy.deepcopy(s1_hi))
    nets["master_rows"].load_state_dict(copy.deepcopy(s1))
    _same_tables(nm, nets["master_rows"], "reloaded master")
    for k in nm.tables:
        assert torch.equal(bits16(nets["bf16"].tables[k]), bits16(nm.tables[k])), k
    feed2 = fuzz_step.make_feed(c, P=max(2, c.P // 2), seed=c.feed_seed + 1)
    _step(nets, feed2, {n: s1_hi[n].to(DEV) for n in TABLES.values()}, False, "step 2")
    return c


def main():
    for i, (pin, seed) in enumerate(CASES):
        one_case(pin, seed, i)
        print("ok   case %d %r" % (i, pin), flush=True)


if __name__ == "__main__":
    main()
