"""Thin torch-tensor front end of the C ABI (include/clsr_hip.h).

``call("clsr_pgemm", X, ldx, ...)`` converts torch tensors to raw device pointers, checks
their dtype against the C prototype, appends nothing: the trailing ``stream`` argument of every
kernel entry point is filled with torch's current HIP stream.  PyTorch is used only as the
owner of device memory and streams.
"""
import collections
import ctypes

import torch

from clsr_amd import _lib


_scope = [None]   # raw stream of the innermost ``stream_scope`` (None: ask torch on every launch)
_scope_obj = [None]


def current_stream():
    """torch's current stream object (cached by the innermost ``stream_scope``)."""
    s = _scope_obj[0]
    return s if s is not None else torch.cuda.current_stream()


def stream_ptr():
    s = _scope[0]
    return s if s is not None else torch.cuda.current_stream().cuda_stream


class stream_scope(object):
    """``with stream_scope(stream=None):`` -- every ``call`` inside launches on ``stream`` (default: torch's current
    stream, looked up ONCE instead of per launch: ``torch.cuda.current_stream()`` costs ~8 us, a step has ~190
    launches).  Nests; code that switches torch's current stream inside a scope opens an inner scope."""

    def __init__(self, stream=None):
        self.stream = stream

    def __enter__(self):
        self.prev = (_scope[0], _scope_obj[0])
        obj = self.stream if self.stream is not None else torch.cuda.current_stream()
        _scope[0], _scope_obj[0] = obj.cuda_stream, obj
        return self

    def __exit__(self, *exc):
        _scope[0], _scope_obj[0] = self.prev
        return False


# ---- launch plans: the host side of a step whose shapes, buffers and scalars do not change is a fixed sequence of
# C-ABI calls and stream-event operations.  Recorded once (while it executes), it is replayed with the arguments
# already converted -- ~2 us per launch instead of ~10-20 us of tensor / dtype checks, descriptor packing, buffer
# look-ups and torch stream queries (clsr_amd/net.py: CLSRNet.train_step / forward).
class LaunchPlan(object):
    __slots__ = ("ops", "keep", "result")

    def __init__(self):
        self.ops, self.keep, self.result = [], [], None


_rec = [None]


def record_begin():
    _rec[0] = LaunchPlan()
    return _rec[0]


def record_end():
    p, _rec[0] = _rec[0], None
    return p


def recording():
    return _rec[0] is not None


def replay(plan):
    for fn, args in plan.ops:
        rc = fn(*args)
        if rc:                      # ctypes entry points return 0 / negative; torch stream methods return None
            _lib.check(rc, getattr(fn, "__name__", "replayed launch"))


def keep_alive(*objs):
    """Descriptor arrays whose ADDRESS is passed to a recorded call must outlive the plan."""
    if _rec[0] is not None:
        _rec[0].keep.extend(objs)


def event_record(stream):
    """A new event recorded on ``stream`` (a torch stream object)."""
    ev = torch.cuda.Event()
    ev.record(stream)
    if _rec[0] is not None:
        _rec[0].ops.append((ev.record, (stream,)))
    return ev


def stream_wait(stream, ev):
    stream.wait_event(ev)
    if _rec[0] is not None:
        _rec[0].ops.append((stream.wait_event, (ev,)))


def host_call(fn, *args):
    """Run a host-side callback now and, while a launch plan is being recorded, make it part of the plan (the
    data-parallel collectives issued from inside a step: clsr_amd/dp.py).  The callback must return None."""
    rec, _rec[0] = _rec[0], None      # launches made by the callback itself belong to the callback, not to the plan
    try:
        fn(*args)
    finally:
        _rec[0] = rec
    if rec is not None:
        rec.ops.append((fn, args))


def call(name, *args, stream=None):
    """Invoke an ``int clsr_*(..., void* stream)`` entry point; raises on a non-zero return."""
    lib = _lib.load()
    fn = getattr(lib, name)
    kinds = fn.ptr_kinds
    if len(args) != len(kinds) - 1:
        raise TypeError("%s expects %d arguments (+stream), got %d" % (name, len(kinds) - 1, len(args)))
    conv = []
    for i, (a, kind) in enumerate(zip(args, kinds)):
        if kind is not None:
            if a is None:
                conv.append(None)
            elif isinstance(a, torch.Tensor):
                if not a.is_cuda:
                    raise TypeError("%s arg %d: tensor must live on the GPU" % (name, i))
                if kind != "void" and str(a.dtype) != "torch." + kind:
                    raise TypeError("%s arg %d: expected %s tensor, got %s" % (name, i, kind, a.dtype))
                conv.append(a.data_ptr())
            elif isinstance(a, int):
                conv.append(a)
            else:
                raise TypeError("%s arg %d: expected tensor/None/address, got %r" % (name, i, type(a)))
        else:
            conv.append(a)
    conv.append(stream if stream is not None else stream_ptr())
    rc = fn(*conv)
    _lib.check(rc, name)
    if _rec[0] is not None:
        _rec[0].ops.append((fn, tuple(conv)))


def query(name, *args):
    """Invoke a pure host-side size query (``clsr_*_parts`` / ``*_workspace_floats``)."""
    return getattr(_lib.load(), name)(*args)


def graph_begin(stream=None):
    lib = _lib.load()
    _lib.check(lib.clsr_graph_begin(stream if stream is not None else stream_ptr()), "clsr_graph_begin")


def graph_end(stream=None):
    lib = _lib.load()
    out = ctypes.c_void_p()
    _lib.check(lib.clsr_graph_end(stream if stream is not None else stream_ptr(), ctypes.byref(out)),
               "clsr_graph_end")
    return out.value


def graph_launch(graph_exec, stream=None):
    lib = _lib.load()
    _lib.check(lib.clsr_graph_launch(graph_exec, stream if stream is not None else stream_ptr()),
               "clsr_graph_launch")


def graph_destroy(graph_exec):
    _lib.check(_lib.load().clsr_graph_destroy(graph_exec), "clsr_graph_destroy")


# ---- descriptor structs (include/clsr_hip.h).  The ctypes classes are GENERATED from the header (_lib.parse_structs):
# field names, order and types have one source.  Structs that travel as lists (the *_multi launches, the dW reduction
# table) also carry ``cls.row``: a namedtuple over the field names, every default 0, pointer fields given as a tensor,
# None or an integer address and stored as integers -- ``ops.ZeroDesc.row(p=buf, nbytes=n)``.  A row is a tuple, so
# positional rows (pointers as integers) stay valid wherever rows are taken; ``desc_array`` packs either kind.
def _addr(v):
    """Tensor / None / integer address -> integer address (any other value passes through)."""
    return 0 if v is None else v.data_ptr() if isinstance(v, torch.Tensor) else v


def _row_type(cls):
    names = cls.names
    ptrs = frozenset(n for n, t in cls._fields_ if t is ctypes.c_void_p)
    base = collections.namedtuple(cls.__name__ + "Row", names, defaults=(0,) * len(names))
    make = base.__new__

    class Row(base):
        __slots__ = ()

        def __new__(c, **kw):      # (an unknown field name: namedtuple's TypeError)
            for k, v in kw.items():
                if k in ptrs and v.__class__ is not int:
                    kw[k] = 0 if v is None else v.data_ptr()
            return make(c, **kw)

    Row.__name__ = Row.__qualname__ = base.__name__
    return Row


def _mirror(pyname, cname, rows=False):
    cls = type(pyname, (ctypes.Structure,), {"_fields_": _STRUCTS[cname], "cname": cname, "names": [n for n, _ in _STRUCTS[cname]],
                                             "__doc__": "ctypes mirror of %s (include/clsr_hip.h)." % cname})
    if rows:
        cls.row = _row_type(cls)
    return cls


_STRUCTS = _lib.parse_structs()
GruDesc, T4Desc = _mirror("GruDesc", "clsr_gru_desc"), _mirror("T4Desc", "clsr_t4_desc")
PackDesc, HeadsDesc = _mirror("PackDesc", "clsr_pack_desc"), _mirror("HeadsDesc", "clsr_heads_desc")
BnPtrs = dict(HeadsDesc._fields_)["bn"]._type_          # clsr_bn_ptrs: the member type of clsr_heads_desc.bn[4]
MarkDesc, ZeroDesc = _mirror("MarkDesc", "clsr_mark_desc", True), _mirror("ZeroDesc", "clsr_zero_desc", True)
ScatterDesc, GatherDesc = _mirror("ScatterDesc", "clsr_scatter_desc", True), _mirror("GatherDesc", "clsr_gather_desc", True)
RpDesc, TableDesc = _mirror("RpDesc", "clsr_rp_desc", True), _mirror("TableDesc", "clsr_table_desc", True)
SortIdsDesc, SegsumDesc = _mirror("SortIdsDesc", "clsr_sortids_desc", True), _mirror("SegsumDesc", "clsr_segsum_desc", True)
DwJob, DwDesc = _mirror("DwJob", "clsr_dwjob", True), _mirror("DwDesc", "clsr_dw_desc", True)

_MULTI_SIZES = ("clsr_mark_desc", "clsr_gather_desc", "clsr_rp_desc", "clsr_table_desc")   # clsr_sizeof_multi_descs
_layout_checked = set()


def check_layout(cls):
    """First use of a descriptor class: its size against the loaded library's answer (a library built from another
    header would read every later field from the wrong place)."""
    if cls in _layout_checked:
        return
    lib = _lib.load()
    if cls.cname in _MULTI_SIZES:
        sz = [ctypes.c_int() for _ in _MULTI_SIZES]
        lib.clsr_sizeof_multi_descs(*[ctypes.byref(x) for x in sz])
        want = sz[_MULTI_SIZES.index(cls.cname)].value
    else:
        want = getattr(lib, "clsr_sizeof_" + cls.cname[len("clsr_"):])()
    if ctypes.sizeof(cls) != want:
        raise RuntimeError("%s: %d bytes in include/clsr_hip.h, %d in %s" % (cls.cname, ctypes.sizeof(cls), want, _lib.LIB_PATH))
    _layout_checked.add(cls)


def desc_array(cls, rows):
    """ctypes array of ``cls`` from rows (``cls.row`` or positional tuples in field order, pointers as integers / None).
    A row shorter than the struct leaves its trailing fields zero; a longer one is an error."""
    check_layout(cls)
    names = cls.names
    arr = (cls * len(rows))()
    for d, row in zip(arr, rows):
        if len(row) > len(names):
            raise TypeError("%s has %d fields, got a row of %d values" % (cls.cname, len(names), len(row)))
        for name, val in zip(names, row):
            setattr(d, name, val)
    return arr


def _desc(cls, **fields):
    """One descriptor that travels by address: the given fields set, tensors as their addresses."""
    check_layout(cls)
    d = cls()
    for name, v in fields.items():
        if v is not None:       # (None: a null pointer, which the fresh descriptor already holds)
            setattr(d, name, v if v.__class__ is int else _addr(v))
    return d


def _upload(arr, device):
    return torch.frombuffer(bytearray(bytes(memoryview(arr))), dtype=torch.uint8).to(device)


# hidden-to-hidden products of the recurrences (clsr_gru_desc.products): process default / fp32-input MFMA / split-bf16
RNN_PRODUCTS = {None: 0, "default": 0, "fp32": 1, "x3": 2, "x6": 3}


def _ptr(t):
    return None if t is None else t.data_ptr()


def gru_desc(n, Pin=None, ldp=0, Wgh=None, ldg=0, Wch=None, ldc=0, h0=None, h0_stride=0, hT=None, out_seq=None,
             hprev=None, gates=None, dhT=None, dout_seq=None, dPin=None, dh0=None, lddp=0, att=None, datt=None,
             in_div=1, products=0, X=None, ldx=0, Dx=0, Wgx=None, Wcx=None, bg=None, bc=None):
    kw = dict(locals())
    kw["products"] = RNN_PRODUCTS.get(products, products)
    return _desc(GruDesc, dpin_bf16=int(dPin is not None and dPin.dtype == torch.bfloat16), **kw)


def t4_desc(n, Pin=None, ldp=0, Wm=None, ldm=0, out_seq=None, act=None, cst=None, mprev=None, dout_seq=None,
            dPin=None, lddp=0, st_in=None, st_out=None, dst_in=None, dst_out=None, products=0, act_tiled=False,
            X=None, ldx=0, Dx=0, Wkx=None, bk=None):
    kw = dict(locals())
    kw.update(products=RNN_PRODUCTS.get(products, products), act_tiled=int(bool(act_tiled)))
    return _desc(T4Desc, dpin_bf16=int(dPin is not None and dPin.dtype == torch.bfloat16), **kw)


def rnn_multi(name, grus, t4, seq_len, len_stride, Hn, T, t_range=None):
    """clsr_rnn_fwd_multi / clsr_rnn_bwd_multi with python lists of descriptors; ``t_range=(t0, t1)``: the
    ``*_range`` entry points (one time range of a recurrence that runs as a chain of launches)."""
    arr = (GruDesc * max(len(grus), 1))(*grus)
    t4p = ctypes.addressof(t4) if t4 is not None else None
    keep_alive(arr, t4, grus)
    if t_range is None:
        call(name, ctypes.addressof(arr) if grus else None, len(grus), t4p, seq_len, len_stride, Hn, T)
    else:
        call(name + "_range", ctypes.addressof(arr) if grus else None, len(grus), t4p, seq_len, len_stride, Hn, T,
             int(t_range[0]), int(t_range[1]))


def pack_desc(src1, O, I, dst, Kp, ld1=None, transposed=False, o0=0, i0=0, src2=None, s1=1.0, s2=1.0, ld2=None):
    return _desc(PackDesc, src1=src1, src2=src2, dst=dst, s1=float(s1), s2=float(s2),
                 ld1=src1.stride(0) if ld1 is None else ld1,
                 ld2=(src2.stride(0) if src2 is not None else 0) if ld2 is None else ld2,
                 transposed=int(bool(transposed)), O=O, I=I, Kp=Kp, o0=o0, i0=i0)


def pack_table(descs, device):
    """Upload a list of PackDesc to device memory; returns (tensor, n, max_elems)."""
    return _upload((PackDesc * len(descs))(*descs), device), len(descs), max(d.O * d.I for d in descs)


def dw_table(sig, device):
    """Upload dW-reduction descriptors (DwDesc rows: partial, dW, db, scale, nparts, K, N, ldw, accumulate[, partial2,
    scale2, nparts2: a second product summed into the same output]) to the device; returns (tensor, n, max_outputs)."""
    arr = desc_array(DwDesc, sig)
    # max_outputs / 64 = blocks per descriptor: one per quarter of a 16 x 16 tile (+ 64-wide bias slices)
    cd = lambda a, b: -(-a // b)
    return _upload(arr, device), len(sig), 64 * max(cd(d.K, 16) * cd(d.N, 16) * 4 + (cd(d.N, 64) if d.db else 0) for d in arr)


def sort_ids_multi(rows):
    """clsr_sort_ids_multi on a list of SortIdsDesc rows (ids, keys_out, perm_out, counts, nrows, row_stride, ncols, bits)."""
    arr = desc_array(SortIdsDesc, rows)
    keep_alive(arr)
    call("clsr_sort_ids_multi", ctypes.addressof(arr), len(rows))


_STABLE_SHORT = ("ids", "keys_out", "perm_out", "nrows", "row_stride", "ncols", "bits", "ids2", "nrows2", "row_stride2")


def sort_ids_stable_multi(rows, workspace):
    """clsr_sort_ids_stable_multi on a list of SortIdsDesc rows, or of the short form without ``counts`` (which this
    sort does not use): (ids, keys_out, perm_out, nrows, row_stride, ncols, bits[, ids2, nrows2, row_stride2]) tuples,
    pointers as integers; ``workspace``: a uint8 tensor of clsr_sort_ids_stable_workspace_bytes(total entries, tables)."""
    full = []
    for r in rows:
        if not isinstance(r, SortIdsDesc.row):
            if len(r) > len(_STABLE_SHORT):
                raise TypeError("clsr_sortids_desc short form has %d fields, got a row of %d values" % (len(_STABLE_SHORT), len(r)))
            r = SortIdsDesc.row(**dict(zip(_STABLE_SHORT, r)))
        full.append(r)
    arr = desc_array(SortIdsDesc, full)
    keep_alive(arr)
    call("clsr_sort_ids_stable_multi", ctypes.addressof(arr), len(rows), workspace, workspace.numel())


def segsum_descs(rows):
    """ctypes array of clsr_segsum_desc from SegsumDesc rows."""
    return desc_array(SegsumDesc, rows)


def segsum_workspace_bytes(rows):
    arr = segsum_descs(rows)
    return query("clsr_segsum_workspace_bytes", ctypes.addressof(arr), len(rows))


def segsum_multi(rows, workspace):
    """clsr_segsum_multi: deterministic segmented sums of the lookup sites ``rows`` into their gradient tables."""
    arr = segsum_descs(rows)
    keep_alive(arr)
    call("clsr_segsum_multi", ctypes.addressof(arr), len(rows), workspace, workspace.numel())


def heads_desc(**kw):
    """clsr_heads_desc from keyword values: tensors become their device pointers, ``bn`` is a list of four dicts."""
    bn = kw.pop("bn")
    d = _desc(HeadsDesc, **kw)
    for i, layer in enumerate(bn):
        for name, v in layer.items():
            setattr(d.bn[i], name, _addr(v))
    return d


def heads_fused(step, desc):
    """clsr_heads_fused_step1 / _step2 on a HeadsDesc."""
    keep_alive(desc)
    call("clsr_heads_fused_step%d" % step, ctypes.addressof(desc))


FEED_COLUMNS = ("item_history", "item_cate_history", "time_from_first_action", "time_to_now", "lens", "users", "items", "cates")
FEED_OUTPUTS = ("users", "items", "cates", "item_history", "item_cate_history", "time_from_first_action", "time_to_now",
                "labels", "seq_len", "denom")


def _feed_pointer_array(entry, names, tensors):
    """The host pointer array of feed entry point ``entry`` from a dict of tensors, in the order of ``names``, with the
    dtypes the entry point reads them as checked here (it sees addresses only).  ``users_rows`` alone may be missing: a
    null pointer."""
    for k, t in tensors.items():
        want = torch.float32 if k in ("time_from_first_action", "time_to_now", "labels", "denom") else torch.int32
        if not (t.is_cuda and t.is_contiguous() and t.dtype == want):
            raise TypeError("%s %s: a contiguous %s GPU tensor is required, got %s" % (entry, k, want, t.dtype))
    missing = [k for k in names if k not in tensors and k != "users_rows"]
    if missing:
        raise KeyError("%s: no tensor %s" % (entry, ", ".join(missing)))
    return (ctypes.c_void_p * len(names))(*[tensors[k].data_ptr() if k in tensors else None for k in names])


def feed_pointers(cols, outs):
    """The two host pointer arrays of clsr_feed_build from dicts of tensors (``FEED_COLUMNS`` / ``FEED_OUTPUTS``)."""
    return (_feed_pointer_array("clsr_feed_build", FEED_COLUMNS, cols),
            _feed_pointer_array("clsr_feed_build", FEED_OUTPUTS, outs))


def feed_build(ptrs, N, sel, n_sel, src, h0, n, T, G, expanded, thr, err):
    """clsr_feed_build: the two launches that build (lines h0 .. h0 + n - 1 of) a training feed from resident columns.
    ``ptrs``: the result of :func:`feed_pointers`; ``sel`` / ``src``: int32 tensors or device addresses."""
    keep_alive(ptrs)
    call("clsr_feed_build", ctypes.addressof(ptrs[0]), N, sel, n_sel, src, h0, n, T, G, int(expanded), thr,
         ctypes.addressof(ptrs[1]), err)


def feed_build_pos(ptrs, N, sel, n_sel, psrc, h0, n, T, G, expanded, thr, scratch, err):
    """clsr_feed_build_pos: the three launches that build (lines h0 .. h0 + n - 1 of) a NextItNet training feed from
    resident columns.  ``ptrs``: the result of :func:`feed_pointers`; ``sel`` / ``psrc`` / ``scratch``
    (``clsr_feed_build_pos_scratch_ints(n_sel)`` ints): int32 tensors or device addresses."""
    keep_alive(ptrs)
    call("clsr_feed_build_pos", ctypes.addressof(ptrs[0]), N, sel, n_sel, psrc, h0, n, T, G, int(expanded), thr,
         ctypes.addressof(ptrs[1]), scratch, err)


FEED_EVAL_COLUMNS = FEED_COLUMNS + ("labels",)
FEED_EVAL_OUTPUTS = ("users", "items", "cates", "item_history", "item_cate_history", "time_from_first_action", "time_to_now",
                     "labels", "users_rows", "seq_len", "denom")


def feed_eval_pointers(cols, outs=None):
    """The host pointer arrays of clsr_feed_same_rows / clsr_feed_build_eval from dicts of tensors (``FEED_EVAL_COLUMNS``;
    ``FEED_EVAL_OUTPUTS``, where ``users_rows`` may be missing: a null pointer), dtypes checked as in
    :func:`feed_pointers`.  ``outs=None``: the column array alone."""
    cp = _feed_pointer_array("clsr_feed_build_eval", FEED_EVAL_COLUMNS, cols)
    return cp if outs is None else (cp, _feed_pointer_array("clsr_feed_build_eval", FEED_EVAL_OUTPUTS, outs))


def feed_same_rows(cols_ptrs, N, keep, n_keep, T, flags):
    """clsr_feed_same_rows: ``flags`` uint8 ``[n_keep]``, 1 where line ``keep[i]`` repeats the history-level columns of
    ``keep[i - 1]``.  ``keep`` must have been checked against ``[0, N)`` by the caller."""
    keep_alive(cols_ptrs)
    call("clsr_feed_same_rows", ctypes.addressof(cols_ptrs), N, keep, n_keep, T, flags)


def feed_build_eval(ptrs, N, keep, n_keep, k0, n, g, T, thr):
    """clsr_feed_build_eval: the one launch that builds the scoring feed of lines ``keep[k0 : k0 + n]`` in groups of ``g``.
    ``ptrs``: the pair :func:`feed_eval_pointers` returns."""
    keep_alive(ptrs)
    call("clsr_feed_build_eval", ctypes.addressof(ptrs[0]), N, keep, n_keep, k0, n, g, T, thr, ctypes.addressof(ptrs[1]))


DW_MULTI_MAX = 12


def dw_multi(name, rows, stream=None):
    """clsr_pgemm_dw_partial_multi / clsr_hdw_partial_multi on a list of DwJob rows."""
    for i in range(0, len(rows), DW_MULTI_MAX):
        arr = desc_array(DwJob, rows[i:i + DW_MULTI_MAX])
        keep_alive(arr)
        call(name, ctypes.addressof(arr), len(arr), stream=stream)


def multi(name, cls, rows, *extra, lo=None):
    """Launch ``name`` (a clsr_*_multi entry point) on a list of ``cls`` rows (chunks of 16).  ``lo``: one
    device address per row, passed as a parallel pointer array behind the descriptors (clsr_tables_adam_multi_hm)."""
    lim = 4 if cls is TableDesc else 16
    for i in range(0, len(rows), lim):
        arr = desc_array(cls, rows[i:i + lim])
        keep_alive(arr)
        if lo is None:
            call(name, ctypes.addressof(arr), len(arr), *extra)
        else:
            ptrs = (ctypes.c_void_p * len(arr))(*lo[i:i + lim])
            keep_alive(ptrs)
            call(name, ctypes.addressof(arr), ctypes.addressof(ptrs), len(arr), *extra)


def kp_for(K):
    """Row stride of a packed transposed weight for an input width K (see clsr_pack_weight)."""
    return 16 * ((K + 15) // 16) + 4


def pack_weight(W, out_features, in_features, transposed=False, W2=None, s1=1.0, s2=1.0, ld=None,
                ld2=None, out=None):
    """Pack a [in, out] weight block (or its transpose) into the MFMA A-operand layout
    Wt[16*ceil(out/16)][Kp], zero padded.  ``W``/``W2`` may be views into larger matrices
    (pass their row stride ``ld``)."""
    Kp = kp_for(in_features)
    opad = 16 * ((out_features + 15) // 16)
    if out is None:
        out = torch.empty(opad * Kp, dtype=torch.float32, device=W.device)
    ld = W.stride(0) if ld is None else ld
    ld2 = (W2.stride(0) if W2 is not None else 0) if ld2 is None else ld2
    call("clsr_pack_weight", W, ld, float(s1), W2, ld2, float(s2), 1 if transposed else 0,
         out_features, in_features, Kp, out)
    return out, Kp
