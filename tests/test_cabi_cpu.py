"""CPU test: the C-ABI shared library builds for gfx950, loads, and exports every symbol that
include/clsr_hip.h declares (no kernel is launched here)."""
import os

from clsr_amd import _lib


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        from clsr_amd.build import build

        build(verbose=False)
    protos = _lib.parse_header()
    assert len(protos) >= 40
    lib = _lib.load()
    for name in protos:
        assert hasattr(lib, name), name
    assert lib.clsr_version() >= 100
    # host-only queries work without a GPU
    assert lib.clsr_pgemm_dw_workspace_floats(1024, 80, 80) > 0
    assert lib.clsr_pgemm_stats_parts(100000) > 0


def test_invalid_arguments_are_reported_not_thrown():
    lib = _lib.load()
    rc = lib.clsr_pgemm(None, 0, 0, 0, None, 0, None, None, 0, None, 0, None, None, 0, None, 0, None, 0, 0,
                        None, 16, 16, 16, None)
    assert rc == -1
    assert "invalid argument" in _lib.last_error()


MIRRORS = {"clsr_gru_desc": "GruDesc", "clsr_t4_desc": "T4Desc", "clsr_pack_desc": "PackDesc", "clsr_dw_desc": "DwDesc",
           "clsr_mark_desc": "MarkDesc", "clsr_zero_desc": "ZeroDesc", "clsr_scatter_desc": "ScatterDesc",
           "clsr_gather_desc": "GatherDesc", "clsr_rp_desc": "RpDesc", "clsr_table_desc": "TableDesc",
           "clsr_sortids_desc": "SortIdsDesc", "clsr_segsum_desc": "SegsumDesc", "clsr_bn_ptrs": "BnPtrs",
           "clsr_heads_desc": "HeadsDesc", "clsr_dwjob": "DwJob"}


def test_descriptor_structs_match_their_ctypes_mirrors():
    """Every descriptor struct that crosses the ABI by address has a ctypes mirror in clsr_amd/ops.py: same size as the C
    side reports (a field added on one side only would shift every later field silently)."""
    import ctypes

    from clsr_amd import ops

    lib = _lib.load()
    assert set(_lib.parse_structs()) == set(MIRRORS)
    multi = [ctypes.c_int() for _ in range(4)]
    lib.clsr_sizeof_multi_descs(*[ctypes.byref(x) for x in multi])
    multi = dict(zip(("clsr_mark_desc", "clsr_gather_desc", "clsr_rp_desc", "clsr_table_desc"), (x.value for x in multi)))
    checked = 0
    for cname, pyname in MIRRORS.items():
        mirror = getattr(ops, pyname)
        assert [n for n, _ in mirror._fields_] == [n for n, _ in _lib.parse_structs()[cname]], cname
        if cname == "clsr_bn_ptrs":     # no query of its own: the library's clsr_heads_desc holds four of them
            assert ops.HeadsDesc.bn.size == 4 * ctypes.sizeof(mirror)
            assert ctypes.sizeof(ops.HeadsDesc) == lib.clsr_sizeof_heads_desc()
        elif cname in multi:
            assert ctypes.sizeof(mirror) == multi[cname], cname
            ops.check_layout(mirror)
        else:
            assert ctypes.sizeof(mirror) == getattr(lib, "clsr_sizeof_" + cname[len("clsr_"):])(), cname
            ops.check_layout(mirror)
        checked += 1
    assert checked == 15
    # host-only queries of the round-4 entry points
    assert lib.clsr_heads_fused_workspace_bytes() > lib.clsr_heads_fused_counter_bytes() > 0
    assert lib.clsr_heads_comm_buffer_bytes() > 0 and lib.clsr_heads_comm_max_world() == 8
    assert lib.clsr_pgemm_dw_wide_supported(204800, 128, 1536) == 1 and lib.clsr_pgemm_dw_wide_supported(204800, 40, 360) == 0
    assert lib.clsr_pgemm_dw_wide_workspace_floats(204800, 128, 1536) >= 128 * 1536
    assert lib.clsr_comm_buffer_bytes() > 0 and lib.clsr_comm_max_doubles() == 256


def _host_cc():
    """$CC, else cc, else the clang that ROCm bundles; none of them: the layout test fails (it never skips)."""
    import shutil

    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    for cand in (os.environ.get("CC"), "cc", rocm_clang):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    raise AssertionError("no host C compiler ($CC, cc, %s)" % rocm_clang)


def test_descriptor_layouts_match_the_c_compiler(tmp_path):
    """sizeof of every descriptor struct and offsetof of every field, as the host C compiler lays the header out, against
    the generated ctypes classes: all 15 structs, every field (sizeof alone does not see two same-sized fields swapped)."""
    import ctypes
    import subprocess

    from clsr_amd import ops

    structs = _lib.parse_structs()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "clsr_hip.h"', 'int main(void) {']
    for cname, fields in structs.items():
        lines.append('  printf("%s  %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in fields:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([_host_cc(), "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        cname, fname, value = line.split(" ")
        got[(cname, fname)] = int(value)
    want = {}
    for cname, pyname in MIRRORS.items():
        mirror = getattr(ops, pyname)
        want[(cname, "")] = ctypes.sizeof(mirror)
        for fname, _ in mirror._fields_:
            want[(cname, fname)] = getattr(mirror, fname).offset
    assert len(MIRRORS) == 15 and got == want


# field names of the structs that travel as lists, in order: positional callers (bench.py among them) depend on it, so a
# reordered header must fail here instead of misplacing a pointer there
LIST_FIELDS = {
    "MarkDesc": ["idx", "flags", "nrows", "row_stride", "ncols", "pad_"],
    "ZeroDesc": ["p", "nbytes"],
    "ScatterDesc": ["src", "idx", "tbl_grad", "sumsq", "idx_stride", "ld_src", "col0", "N", "C"],
    "GatherDesc": ["table", "idx", "out", "idx_stride", "N", "C", "ldo", "col0"],
    "RpDesc": ["partial", "out", "scale", "nparts", "stride", "n", "accumulate", "pad_"],
    "TableDesc": ["table", "partner", "grad", "m", "v", "flags", "sumsq_reg", "disc_loss", "sumsq_adam", "V", "C", "nsum",
                  "sumsq_stride", "disc_scale", "disc_loss_scale", "pad_"],
    "SortIdsDesc": ["ids", "keys_out", "perm_out", "counts", "nrows", "row_stride", "ncols", "bits", "ids2", "nrows2",
                    "row_stride2"],
    "SegsumDesc": ["src", "src2", "dmean", "drecent", "keys", "perm", "seq_len", "grad", "sumsq", "n", "src_bf16",
                   "len_stride", "T", "D", "col0", "C", "recent_k", "ldg", "gcol0", "assign", "src_b", "sumsq_b", "n1", "ldb",
                   "colb", "border_wch", "pad_"],
    "DwJob": ["X", "Xmul", "in_scale", "in_shift", "dY", "workspace", "x_bf16", "ldx", "T", "G", "ldmul", "in_relu",
              "dy_bf16", "ldy", "M", "K", "N", "pad_", "rm_tc", "rm_T", "rm_t0", "pgx", "pstride", "poff"],
    "DwDesc": ["partial", "dW", "db", "scale", "nparts", "K", "N", "ldw", "accumulate", "partial2", "scale2", "nparts2"],
}


def test_positional_field_order_is_frozen():
    from clsr_amd import ops

    assert {name: [n for n, _ in getattr(ops, name)._fields_] for name in LIST_FIELDS} == LIST_FIELDS
    for name in LIST_FIELDS:
        assert list(getattr(ops, name).row._fields) == LIST_FIELDS[name]


def _raw(arr):
    return bytes(memoryview(arr))


def test_named_rows_pack_like_positional_tuples():
    """A named row and the positional tuple of the same values give byte-identical descriptor arrays, for every struct
    that travels as a list (CPU tensors: only their addresses are used)."""
    import ctypes

    import pytest
    import torch

    from clsr_amd import ops

    t = [torch.zeros(8) for _ in range(12)]
    p = [x.data_ptr() for x in t]
    # pointer fields take the tensors t[0], t[1], ... in field order, the other fields distinct non-zero numbers
    for name, fields in LIST_FIELDS.items():
        cls = getattr(ops, name)
        named, flat, k = {}, [], 0
        for i, (fname, ctype) in enumerate(cls._fields_):
            if ctype is ctypes.c_void_p:
                named[fname], val = t[k], p[k]
                k += 1
            else:
                named[fname] = val = (i + 1.5) if ctype in (ctypes.c_float, ctypes.c_double) else i + 3
            flat.append(val)
        row = cls.row(**named)
        assert tuple(row) == tuple(flat) and len(row) == len(fields)
        assert _raw(ops.desc_array(cls, [row, row])) == _raw(ops.desc_array(cls, [tuple(flat), flat]))
        assert _raw(ops.desc_array(cls, [row])) != bytes(ctypes.sizeof(cls))

    # the benchmark's full item-site row of the segmented sums, written positionally as bench.py writes it
    ne, n, bf, G, T, D, Di = 1000, 900, 1, 5, 50, 40, 32
    pad = lambda v: v + (0,) * (6 - len(v))
    for merged in (True, False):
        tail_i = (1, p[9], p[10], n, D, 0) if merged else (0,)
        bench_row = (p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], ne, bf, G, T, D, 0, Di, 3, Di, 0) + pad(tail_i) + (0, 0)
        second = dict(assign=1, src_b=t[9], sumsq_b=t[10], n1=n, ldb=D) if merged else {}
        row = ops.SegsumDesc.row(src=t[0], src2=t[1], dmean=t[2], drecent=t[3], keys=t[4], perm=t[5], seq_len=t[6], grad=t[7],
                                 sumsq=t[8], n=ne, src_bf16=bf, len_stride=G, T=T, D=D, C=Di, recent_k=3, ldg=Di, **second)
        assert len(bench_row) == len(ops.SegsumDesc._fields_) and row == bench_row
        assert _raw(ops.segsum_descs([row])) == _raw(ops.segsum_descs([bench_row]))

    # short rows: the trailing fields stay zero
    short = ops.desc_array(ops.SegsumDesc, [(p[0], 0, 0, 0, p[4], p[5], 0, p[7], p[8], 7)])
    assert short[0].src == p[0] and short[0].n == 7
    assert _raw(short)[ops.SegsumDesc.src_bf16.offset:] == bytes(ctypes.sizeof(ops.SegsumDesc) - ops.SegsumDesc.src_bf16.offset)
    assert _raw(short) == _raw(ops.desc_array(ops.SegsumDesc, [ops.SegsumDesc.row(src=t[0], keys=t[4], perm=t[5], grad=t[7],
                                                                                 sumsq=t[8], n=7)]))
    # a row that is too long, an unknown field
    with pytest.raises(TypeError, match="clsr_zero_desc has 2 fields, got a row of 3 values"):
        ops.desc_array(ops.ZeroDesc, [(p[0], 16, 0)])
    with pytest.raises(TypeError):
        ops.ZeroDesc.row(p=t[0], nbites=16)
    # None: a null pointer, by name and by position
    assert ops.ZeroDesc.row(p=None, nbytes=4) == (0, 4)
    for arr in (ops.desc_array(ops.ZeroDesc, [ops.ZeroDesc.row(p=None, nbytes=4)]), ops.desc_array(ops.ZeroDesc, [(None, 4)])):
        assert arr[0].p is None and arr[0].nbytes == 4
    # rows are hashable; equal rows hash equal (keys of the dW descriptor-table cache)
    a = ops.DwDesc.row(partial=t[0], dW=t[1], scale=1.0, nparts=4, K=16, N=32, ldw=32)
    b = ops.DwDesc.row(partial=p[0], dW=p[1], db=None, scale=1.0, nparts=4, K=16, N=32, ldw=32, accumulate=0)
    assert a == b and hash(a) == hash(b) and {(a,): 1}[(b,)] == 1
    assert a != ops.DwDesc.row(partial=t[0], dW=t[1], scale=1.0, nparts=4, K=16, N=32, ldw=32, accumulate=1)


def test_stable_sort_short_form_maps_onto_the_full_descriptor(monkeypatch):
    """ops.sort_ids_stable_multi takes SortIdsDesc rows or the 7- / 10-value form without ``counts``: both reach the launch
    as the same bytes."""
    import ctypes

    import pytest
    import torch

    from clsr_amd import ops

    t = [torch.zeros(8, dtype=torch.int32) for _ in range(4)]
    p = [x.data_ptr() for x in t]
    sent = []
    monkeypatch.setattr(ops, "call", lambda name, addr, n, ws, nbytes: sent.append(
        (name, ctypes.string_at(addr, n * ctypes.sizeof(ops.SortIdsDesc)), n, nbytes)))
    ws = torch.zeros(64, dtype=torch.uint8)
    ops.sort_ids_stable_multi([(p[0], p[1], p[2], 8, 1, 1, 5), (p[0], p[1], p[2], 4, 2, 1, 5, p[3], 3, 1)], ws)
    ops.sort_ids_stable_multi([ops.SortIdsDesc.row(ids=t[0], keys_out=t[1], perm_out=t[2], nrows=8, row_stride=1, ncols=1, bits=5),
                               ops.SortIdsDesc.row(ids=t[0], keys_out=t[1], perm_out=t[2], nrows=4, row_stride=2, ncols=1, bits=5,
                                                   ids2=t[3], nrows2=3, row_stride2=1)], ws)
    ops.sort_ids_stable_multi([(p[0], p[1], p[2], 8, 1, 1, 5)], ws)
    assert sent[0] == sent[1] == ("clsr_sort_ids_stable_multi", sent[0][1], 2, 64)
    full = ops.desc_array(ops.SortIdsDesc, [(p[0], p[1], p[2], None, 8, 1, 1, 5, None, 0, 0), (p[0], p[1], p[2], None, 4, 2, 1, 5, p[3], 3, 1)])
    assert sent[0][1] == _raw(full) and sent[2][1] == _raw(full)[:ctypes.sizeof(ops.SortIdsDesc)]
    with pytest.raises(TypeError):
        ops.sort_ids_stable_multi([(p[0], p[1], p[2], 8, 1, 1, 5, p[3], 3, 1, 0)], ws)


def test_an_unknown_member_type_is_an_error(tmp_path):
    import pytest

    h = tmp_path / "x.h"
    h.write_text("typedef struct clsr_a { const float* p; int n; } clsr_a;\n"
                 "typedef struct clsr_b { clsr_a a[2]; long m; short s; } clsr_b;\n")
    with pytest.raises(ValueError, match="clsr_b.s: unknown type 'short'"):
        _lib.parse_structs(str(h))
    h.write_text("typedef struct clsr_a { const float* p; int n; } clsr_a;\n"
                 "typedef struct clsr_b { clsr_a a[2]; long m; } clsr_b;\n")
    got = _lib.parse_structs(str(h))
    assert [n for n, _ in got["clsr_b"]] == ["a", "m"] and got["clsr_b"][0][1]._length_ == 2
