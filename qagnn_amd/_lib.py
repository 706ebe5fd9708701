"""ctypes binding of libqagnn_hip.so, generated from include/*.h by _abi.py, + a thin tensor-level wrapper.

PyTorch is used here for exactly three things: device memory (torch.empty), the current HIP stream handle and
raw data pointers.  All compute goes through the C ABI.  There is no fallback: if the shared library is missing
or no MI355X is visible, `HipKernels()` raises.
"""
import ctypes as C
import functools
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('QAGNN_LIB') or os.path.join(_HERE, 'libqagnn_hip.so')  # QAGNN_LIB: an alternate build (kernel A/B runs)

_H = _abi.headers()  # the ABI as include/*.h state it: prototypes, structs and constants are read there and declared nowhere else
_MAIN = _H['qagnn_hip.h']
EXPORTS = _MAIN.names
EXPORTS_TN = _H['qagnn_hip_tn.h'].names            # the live-tile weight gradient
EXPORTS_INFER = _H['qagnn_hip_infer.h'].names      # the forward-only (evaluation) path
EXPORTS_LOSS = _H['qagnn_hip_loss.h'].names        # the training losses
EXPORTS_EXPLAIN = _H['qagnn_hip_explain.h'].names  # the detailed evaluation: attention export and its trace from the context node
EXPORTS_DEFER = _H['qagnn_hip_defer.h'].names      # the stack backward that finishes dEkEm and db1 of all layers after its last hop
EXPORTS_ROWS = _H['qagnn_hip_rows.h'].names        # the trainable entity table's gradient: row grouping, segment sums, row scatter
EXPORTS_DUAL = _H['qagnn_hip_dual.h'].names        # the two-output NN product: a hop's dX and dS from one pass over dK|dM|dQ
ROWS_CHUNK, ROWS_MAX_N, ROWS_MAX_TABLE = (_H['qagnn_hip_rows.h'].define('QAGNN_ROWS_' + n) for n in ('CHUNK', 'MAX_N', 'MAX_TABLE'))
DEFER_MAX_HOPS = _H['qagnn_hip_defer.h'].define('QAGNN_DEFER_MAX_HOPS')
TRACE_MAX_N = _H['qagnn_hip_explain.h'].define('QAGNN_TRACE_MAX_N')
LOSS_KINDS = {k: _H['qagnn_hip_loss.h'].define('QAGNN_LOSS_' + k.upper()) for k in ('cross_entropy', 'margin_rank')}
LOSS_THREADS = _H['qagnn_hip_loss.h'].define('QAGNN_LOSS_THREADS')
CLS_SLICES, GATHER_MAX, HOP_AMAX_WORDS = (_MAIN.define('QAGNN_' + n) for n in ('CLS_SLICES', 'GATHER_MAX', 'HOP_AMAX_WORDS'))
HOP_AM_X, HOP_AM_S, HOP_AM_AGGR, HOP_AM_H1, HOP_AM_Y, HOP_AM_DOUT, HOP_AM_DH1, HOP_AM_DKMQ = (
    _MAIN.define('QAGNN_HOP_AM_' + n) for n in ('X', 'S', 'AGGR', 'H1', 'Y', 'DOUT', 'DH1', 'DKMQ'))  # the words of qagnn_hop_args.amax in use
qagnn_graph, qagnn_store, qagnn_gather_tabs, qagnn_pack_desc, qagnn_gemm_nn_args, qagnn_hop_args = (
    _MAIN.structs[n] for n in ('qagnn_graph', 'qagnn_store', 'qagnn_gather_tabs', 'qagnn_pack_desc', 'qagnn_gemm_nn_args', 'qagnn_hop_args'))
ABI_VERSION = 25  # bumped when the ABI of include/qagnn_hip.h changes (2: qagnn_graph.tgt_t; 3: (group, class) class order; 4: qagnn_hop_args.accumulate_dX; 5: qagnn_graph_from_blobs; 6: qagnn_edge_attn_fwd_lds_f32 replaces the first LDS kernel; 7: qagnn_graph.pk_s / pk_t / sub_ncls / sub_cls; 8: qagnn_hop_args.gemm_split; 9: qagnn_stack_{fwd,bwd}_f32; 10: qagnn_node_prep_f32 checks the concept ids; 11: qagnn_graph_from_blobs takes an edge CAPACITY, seed epoch, column statistics in the GEMM epilogue, LDS-resident edge forward removed; 12: qagnn_hop_args.side_stream, two buffer sets in the backward workspace; 13: qagnn_gemm_tn2_f32; 14: qagnn_gemm_nn_split_ws_f32 / qagnn_gemm_nn_pack_bytes, hop workspaces carry the pack buffer, qagnn_gemm_nn_prepack_{bytes,f32,clear}; 15: qagnn_head_post_{fwd,bwd}_f32, qagnn_add_row0_f32, qagnn_gather_multi{,_sum}_f32; 16: qagnn_gemm_nn_ws_bytes; 17: the three-MFMA GEMM form -- qagnn_gemm_nn_args.a_amax1 / a_amax2, qagnn_pack_desc.pieces, qagnn_hop_args.amax, qagnn_absmax_f32, qagnn_zero_words, qagnn_gemm_tn_h2_f32; 18: qagnn_hop_args.x_amax / s_amax, qagnn_gelu_dropout_fwd_amax_f32, qagnn_timing_enable / qagnn_timing_read; 19: the reduced-precision form on request -- qagnn_gemm_nn_args.pieces, qagnn_gemm_tn_h1_f32, qagnn_hop_args.gemm_split == 3; 20: qagnn_gelu_dropout_bwd_amax_f32; 21: qagnn_gemm_nn_args.a_rows; 22: qagnn_packed_min_rows; 23: gradient clipping -- qagnn_grad_norm_workspace_elems, qagnn_grad_norm_f32, qagnn_scale_multi_f32, qagnn_radam_step_scaled_f32; 24: qagnn_graph_prep_cap -- the int64 edge-list protocol with an edge CAPACITY; 25: qagnn_store, qagnn_store_gather, qagnn_graph_from_store -- the dataset's graphs resident on the device)


def load_library(path=LIB_PATH):
    """dlopen the C-ABI library and declare every prototype of the headers.  Raises OSError if it has not been built, or lacks one."""
    if not os.path.exists(path):
        raise OSError(f'{path} not found: build it with `python -m qagnn_amd.build` (hipcc, gfx950)')
    lib = C.CDLL(path)
    for hdr, h in _H.items():
        for name, restype, argtypes in h.prototypes:
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise OSError(f'{path} does not export {name}, which include/{hdr} declares: rebuild it with `python -m qagnn_amd.build --force`') from None
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def dual_args(A, lda, M, K, a_amax, C1, ldc1, No1, C2, ldc2, No2, accumulate1=False, accumulate2=False):
    """the two argument blocks of qagnn_gemm_nn_dual_f32 / qagnn_gemm_nn_dual_query from raw addresses (the query needs no device)"""
    out = []
    for Cp, ldc, No, acc in ((C1, ldc1, No1, accumulate1), (C2, ldc2, No2, accumulate2)):
        a = qagnn_gemm_nn_args()
        a.A1, a.lda1, a.K1, a.C, a.ldc, a.M, a.No, a.accumulate, a.a_amax1 = A, lda, K, Cp, ldc, M, No, 1 if acc else 0, a_amax
        out.append(a)
    return out


def choice_loss_bound(kind, nc, Q, max_abs=1.0, margin=0.0, weight=1.0, threads=LOSS_THREADS):
    """(loss bound, gradient bound) of qagnn_choice_loss_f32 as include/qagnn_hip_loss.h states them: absolute errors against exact arithmetic
    on the fp32 inputs.  max_abs: max |x| over the logits; weight: the weight word."""
    import math
    u, v = 2.0 ** -24, 2.0 ** -53
    M, L, w = max(1.0, float(max_abs)), math.log(nc), abs(float(weight))
    S = -(-Q // threads) + math.log2(threads) + nc
    if LOSS_KINDS[kind] == 0:
        return w * M * (u * (nc + 8 + 5 * L) + v * S * (2 + L)), w / Q * u * (nc + 8 + L)
    return w * M * (3 * u + v * S) * (2 + abs(float(margin)) / M), w / Q * 2 * u


def _running_fields(running):
    """running = (run_mean [d], run_var [d], num_batches_tracked or None, dense_pos [d], momentum, unbias) or None -> the same as the C
    ABI takes it: four addresses, d, momentum, unbias (None: no running-statistics update)."""
    if running is None:
        return None, None, None, None, 0, 0.0, 1.0
    rm, rv, nbt, pos, mom, unb = running
    assert rm.is_contiguous() and rv.is_contiguous() and pos.dtype == torch.long and (nbt is None or nbt.dtype == torch.long)
    return rm.data_ptr(), rv.data_ptr(), _ptr(nbt), pos.data_ptr(), rm.numel(), float(mom), float(unb)


def _chk2d(t, name, dtype=torch.float32):
    assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.is_contiguous(), \
        f'{name}: need a contiguous 2-D {dtype} device tensor, got {tuple(t.shape)} {t.dtype} {t.device}'
    return t


def _chkp(t, name):
    """A 2-D fp32 operand of an entry point that takes a row pitch (include/qagnn_hip.h): contiguous, or a view whose rows are contiguous,
    at least their width apart, a multiple of 4 floats apart and 16-byte aligned.  (The natively sequenced hops take no pitches: their
    operands stay with _chk2d.)"""
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2, f'{name}: need a 2-D float32 device tensor, got {tuple(t.shape)} {t.dtype} {t.device}'
    assert t.is_contiguous() or (t.stride(1) == 1 and (t.size(0) == 1 or (t.stride(0) >= t.size(1) and t.stride(0) % 4 == 0)) and t.data_ptr() % 16 == 0), \
        f'{name}: rows must be contiguous, a multiple of 4 floats (and at least their width) apart and 16-byte aligned; got strides {t.stride()} for {tuple(t.shape)}'
    return t


def _ld(t):
    """the row pitch handed to the library for a 2-D operand (a one-row tensor's stride(0) is arbitrary: its width)"""
    return t.size(1) if t.size(0) == 1 else t.stride(0)


def _chkp3(t, name):
    """[B, n, Cc] node rows of the pooling head, i.e. [B * n, ld] with one row pitch ld = _ld3(t) >= Cc"""
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3, f'{name}: need a 3-D float32 device tensor'
    B, n, Cc = t.shape
    ld = _ld3(t)
    assert t.is_contiguous() or (t.stride(2) == 1 and ld >= Cc and ld % 4 == 0 and (B == 1 or t.stride(0) == n * ld) and t.data_ptr() % 16 == 0), \
        f'{name}: need [B, n, Cc] rows with one pitch (a multiple of 4 floats, >= Cc), 16-byte aligned; got strides {t.stride()} for {tuple(t.shape)}'
    return t


def _ld3(t):
    B, n, Cc = t.shape
    return t.stride(1) if n > 1 else (t.stride(0) if B > 1 else Cc)


VALIDATE = os.environ.get('QAGNN_VALIDATE', '0') == '1'  # synchronous input validation (debugging corrupt batches)


class _ErrWatch:
    """Surfaces the device-side input-validation flag of qagnn_graph_prep (err[0]: an edge endpoint, relation id or node type
    was out of range and has been clamped) without a host synchronisation on the hot path.

    The reference raises on such input in its one-hot / index ops (modeling_qagnn.py:352-367, 419-433).  Here the four flag words
    are copied to pinned host memory right behind the preparation kernels, and looked at when the NEXT batch is prepared (or at
    `poll(block=True)`, e.g. at the end of an epoch): a corrupt batch raises one step late instead of training silently on a
    clamped graph.  QAGNN_VALIDATE=1 checks synchronously, in the call that saw the bad batch."""

    def __init__(self):
        self.pending = []
        self.sink = None  # while a hipGraph is being captured (graphed.GraphedStep): the flag tensors the captured launches write

    def watch(self, flags, what, reset=None):
        """`reset`: a persistent flag tensor to clear once its error has been reported (per-call flag arrays need none)."""
        if torch.cuda.is_current_stream_capturing():
            # no copy / event inside a capture; the capturing step keeps the (static) flag tensors and hands them to after_replay()
            # behind every replay, so a bad batch raises one step late under replay exactly as it does on the eager path
            if self.sink is not None:
                self.sink.append((flags, what, reset))
            return
        self.after_replay([(flags, what, reset)])

    def after_replay(self, watched):
        """The flag words of (flags, what, reset) entries -> pinned host memory (async) + an event each: what watch() does for one eager
        call, and what a capturing step does behind graph.replay() for the flag words the replayed launches wrote."""
        for flags, what, reset in watched:
            host = torch.empty(4, dtype=torch.int32, pin_memory=True)
            host.copy_(flags, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.pending.append((ev, host, what, reset))
        if VALIDATE:
            self.poll(block=True)

    def poll(self, block=False):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return  # event queries are not legal while a hipGraph is being captured; the flags are looked at by the next eager call
        keep, bad = [], None
        for ev, host, what, reset in self.pending:
            if block:
                ev.synchronize()
            if not ev.query():
                keep.append((ev, host, what, reset))
            elif int(host[0]) != 0:
                if reset is not None:
                    reset.zero_()
                if bad is None:
                    bad = what
        self.pending = keep
        if bad is not None:
            raise RuntimeError(f'out-of-range input in {bad}: the device replaced it by a safe value; the results of that batch '
                               'are not the reference\'s (which raises in its one-hot / index ops)')


ERR_WATCH = _ErrWatch()


class HipGraph:
    """Device-side prepared graph (see qagnn_graph in include/qagnn_hip.h)."""

    def __init__(self, storage, cstruct, N, E, R, T, block_n=0):
        self.storage, self.c = storage, cstruct
        self.N, self.E, self.Ep, self.R, self.T = N, E, E + N, R, T
        self.block_n = block_n
        self.dynamic = False
        self.C = R * T * T + T
        self.max_chunks = cstruct.max_chunks

    def array(self, name, length):
        """int32 view of one of the struct's arrays (for tests and attention-weight export)."""
        off = (getattr(self.c, name) - self.storage.data_ptr()) // 4
        return self.storage[off:off + length]

    def live_tiles(self):
        """(live_tiles [T], live_list [T], n_live [1]) of the T = ceil(N / 32) k-tiles: int32 views of the words behind err
        (include/qagnn_hip_tn.h)"""
        T = (self.N + 31) // 32
        T4 = (T + 3) // 4 * 4
        w = self.array('err', 16 + 4 + 2 * T4)[16:]
        return w[4:4 + T], w[4 + T4:4 + T4 + T], w[:1]

    def live_classes(self):
        """(live_cls [C], n_live [1]): the classes with an edge in this batch, ascending in live_cls[:n_live] -- int32 views of the words
        behind the live k-tiles (include/qagnn_hip_defer.h; the class reduction of the edge backward gives blocks to these only)"""
        T4 = ((self.N + 31) // 32 + 3) // 4 * 4
        w = self.array('err', 16 + 4 + 2 * T4 + 4 + self.C)[16 + 4 + 2 * T4:]
        return w[4:4 + self.C], w[:1]

    @property
    def cls_part_rows(self):
        """rows of the class-partial scratch of the edge backward (qagnn_edge_attn_bwd_f32's cls_part, qagnn_hop_bwd_workspace_elems)"""
        return self.max_chunks + CLS_SLICES * self.C

    @property
    def cls_count(self):
        return self.array('cls_count', self.C)

    @property
    def eid_s(self):
        return self.array('eid_s', self.Ep)


def _device_of(args, kwargs):
    """Device of the first device tensor (or prepared graph) among the arguments of a kernel call."""
    for a in list(args) + list(kwargs.values()):
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                return a.device
        elif isinstance(a, HipGraph):
            return a.storage.device
        elif isinstance(a, (tuple, list)):
            for t in a:
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    return t.device
    return None


def _on_operand_device(fn):
    """Run a kernel call with the operands' device current, on THAT device's current stream.

    The reference places the LM encoder on cuda:0 and the decoder on cuda:1 whenever two GPUs are visible
    (reference qagnn.py:133-134, 168-169), so the process's current device is not, in general, the device that holds the
    decoder's tensors.  A kernel launched on device 0's stream with device-1 pointers would fault or race with the torch ops
    queued on cuda:1's stream; every entry point of the provider therefore switches to the operands' device first (a no-op
    costing one integer compare when it already is the current one)."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        dev = _device_of(args, kwargs)
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(self, *args, **kwargs)
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)
    return wrapped


class _GuardedMeta(type):
    def __new__(mcls, name, bases, ns):
        for k, v in list(ns.items()):
            if callable(v) and not k.startswith('_'):
                ns[k] = _on_operand_device(v)
        return super().__new__(mcls, name, bases, ns)


class HipKernels(metaclass=_GuardedMeta):
    """Tensor-level calls into libqagnn_hip.so, each on the current HIP stream of the device that holds its operands
    (see _on_operand_device)."""
    name = 'hip'
    infer_attn = True  # stack_infer(attn=True): an `a` buffer per hop for ops.attention_capture
    tn_live = True  # the native hop hands its graph to the dWx_t | dWs_t product (live k-tiles, gemm_tn_graph): ops.hop_bwd_composed follows

    def __init__(self):
        if not torch.cuda.is_available():
            raise RuntimeError('qagnn_amd needs an MI355X: torch.cuda.is_available() is False and there is no CPU fallback')
        self.lib = load_library()
        if self.lib.qagnn_abi_version() != ABI_VERSION:
            raise RuntimeError('libqagnn_hip.so ABI version mismatch')
        # NN GEMMs on the bf16 matrix cores by exact 3-way operand splitting (qagnn_gemm_nn_split_f32) whenever the caller also
        # hands over B in its [No, K] layout; QAGNN_GEMM_SPLIT=0 pins the fp32-MFMA kernels
        # 2 (default): additionally the THREE-MFMA form (scaled two-piece fp16 split, csrc/gemm_nn2.hip) wherever the operand maxima are
        # known -- inside the natively sequenced hops; 1 pins the exact 3 x bf16 split everywhere; 3 asks for the REDUCED-PRECISION form
        # (ONE fp16 MFMA per product where 2 takes three: the GEMM arithmetic of the reference under its --fp16 autocast; never a default)
        self.gemm_split = {'0': 0, '1': 1, '3': 3}.get(os.environ.get('QAGNN_GEMM_SPLIT', '2'), 2)
        self.PACK_MIN_M = int(self.lib.qagnn_packed_min_rows(-1))  # (the library's own threshold: nn2_packed_ok, hop_h2; packed_min_rows)
        self._side_streams = {}  # per device: the stream the natively sequenced hops put their weight-gradient products on
        self._loss_flags = {}    # per device: the bad-label flag word of choice_loss

    # -- helpers -----------------------------------------------------------------------------------------------
    def _stream(self):
        # raw handle of the current device's current stream (torch.cuda.current_stream() builds a Stream object: ~10 us per call,
        # 25 calls per step); the entry points run under _on_operand_device, so "current device" is the operands' device
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())

    def _side_stream(self):
        dev = torch.cuda.current_device()
        st = self._side_streams.get(dev)
        if st is None:
            st = self._side_streams[dev] = torch.cuda.Stream(device=dev)
        return st.cuda_stream

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f'{what} failed (code {rc}): {self.lib.qagnn_last_error().decode()}')

    # -- graph -------------------------------------------------------------------------------------------------
    def _graph_alloc(self, N, E, R, T, device, storage=None):
        """-> (storage, g): int32 device storage for the arrays of a graph of N node rows laid out for E edges -- the caller's, if it is
        large enough, else allocated -- and the struct the builder fills in."""
        elems = self.lib.qagnn_graph_storage_elems(N, E, R, T)
        if storage is None:
            storage = torch.empty(elems, dtype=torch.int32, device=device)
        assert storage.is_cuda and storage.dtype == torch.int32 and storage.is_contiguous() and storage.numel() >= elems
        return storage, qagnn_graph()

    def _graph_done(self, rc, entry, storage, g, N, E, R, T, block_n, dynamic, keep, what):
        """The builders' common tail.  dynamic: E / Ep are capacities, the true E' lives on the device (rowptr_s[N] = sum of cls_count);
        keep: what the kernels just enqueued read; what: the batch, as a reported validation flag names it."""
        self._check(rc, entry)
        G = HipGraph(storage, g, N, E, R, T, block_n)
        G.dynamic, G.keep = dynamic, keep
        ERR_WATCH.poll()  # flags of earlier batches that have landed since
        ERR_WATCH.watch(G.array('err', 4), f'the graph of {what}')
        return G

    @staticmethod
    def _block_n(block_n, N):
        """the sorting builders' block size: 0 (no block structure promised) unless it divides the node rows"""
        return int(block_n) if block_n and N % block_n == 0 else 0

    def graph_prep(self, edge_index, edge_type, node_type, n_etype, n_ntype, block_n=0):
        """block_n = n > 0: the caller expects subgraph i to own node rows [i*n, (i+1)*n) (LM_QAGNN.batch_graph); whether the
        edges really respect that is recorded in a device flag and decides, on the device, which edge kernel runs."""
        assert edge_index.dtype == torch.long and edge_type.dtype == torch.long and node_type.dtype == torch.long
        assert edge_index.dim() == 2 and edge_index.size(0) == 2
        edge_index, edge_type, node_type = edge_index.contiguous(), edge_type.contiguous(), node_type.contiguous()
        N, E = node_type.numel(), edge_index.size(1)
        storage, g = self._graph_alloc(N, E, n_etype, n_ntype, node_type.device)
        block_n = self._block_n(block_n, N)
        rc = self.lib.qagnn_graph_prep_blocked(C.byref(g), storage.data_ptr(), _ptr(edge_index) if E else None,
                                               _ptr(edge_type) if E else None, node_type.data_ptr(), N, E, n_etype, n_ntype,
                                               block_n, self._stream())
        return self._graph_done(rc, 'qagnn_graph_prep_blocked', storage, g, N, E, n_etype, n_ntype, block_n, False, None,
                                f'the batch with N={N} node rows, E={E} edges (edge endpoint / relation id / node type)')

    def graph_prep_cap(self, batch, node_type, n_etype, n_ntype, block_n=0, storage=None):
        """batch: data_utils.EdgeListBatch on the device with a capacity (batch.e_cap >= batch.E; edge_index [2, >= e_cap], edge_type
        [>= e_cap], the count word batch.count).  graph_prep() with the arrays laid out for e_cap edges and the true count read on the
        device (qagnn_graph_prep_cap): every launch shape depends on (N, e_cap) only, entries [E, e_cap) of the buffers are not read.
        storage: int32 device storage of at least qagnn_graph_storage_elems(N, e_cap, ...) elements to build into (else allocated)."""
        ei, et, cnt = batch.edge_index, batch.edge_type, batch.count
        assert ei.is_cuda and et.is_cuda and ei.dtype == torch.long and et.dtype == torch.long and node_type.dtype == torch.long
        assert ei.dim() == 2 and ei.size(0) == 2 and ei.stride(1) == 1 and et.is_contiguous() and node_type.is_contiguous()
        assert cnt is not None and cnt.is_cuda and cnt.dtype == torch.int32 and cnt.numel() == 1, 'EdgeListBatch.count: a one-element int32 device tensor'
        N, E, e_cap = node_type.numel(), int(batch.E), int(batch.e_cap)
        assert 0 <= E <= e_cap, f'edge capacity {e_cap} below the batch\'s {E} edges'
        assert ei.size(1) >= e_cap and et.numel() >= e_cap, f'edge buffers of {ei.size(1)} / {et.numel()} entries below the capacity {e_cap}'
        ld = ei.stride(0) if ei.size(1) > 1 else ei.size(1)
        storage, g = self._graph_alloc(N, e_cap, n_etype, n_ntype, node_type.device, storage)
        block_n = self._block_n(block_n, N)
        rc = self.lib.qagnn_graph_prep_cap(C.byref(g), storage.data_ptr(), ei.data_ptr(), ld, et.data_ptr(), node_type.data_ptr(), N, e_cap,
                                           cnt.data_ptr(), n_etype, n_ntype, block_n, self._stream())
        return self._graph_done(rc, 'qagnn_graph_prep_cap', storage, g, N, e_cap, n_etype, n_ntype, block_n, True, (ei, et, cnt),
                                f'the edge-list batch with N={N} node rows, E={E} edges (edge endpoint / relation id / node type)')

    def graph_from_blobs(self, packed, node_type):
        """packed: data_utils.PackedGraphBatch on the device (the batch's load-time blobs); node_type [B*n] int64.
        packed.e_cap (optional, >= packed.E): lay the arrays out for that many edges -- every launch shape of the step then depends
        on (B, n, e_cap) only and the true count is read on the device, which is what lets one captured hipGraph serve all batches
        of a capacity bucket (qagnn_amd.graphed)."""
        assert packed.buf.is_cuda and packed.buf.dtype == torch.int32 and node_type.dtype == torch.long and node_type.is_contiguous()
        B, n, R, T = packed.B, packed.n, packed.n_etype, packed.n_ntype
        E = packed.E if packed.e_cap is None else int(packed.e_cap)
        assert E >= packed.E, f'edge capacity {E} below the batch\'s {packed.E} edges'
        N = B * n
        assert node_type.numel() == N
        storage, g = self._graph_alloc(N, E, R, T, node_type.device)
        base = packed.buf.data_ptr()
        rc = self.lib.qagnn_graph_from_blobs(C.byref(g), storage.data_ptr(), base + 4 * packed.head, base, base + 4 * (B + 1),
                                             node_type.data_ptr(), B, n, E, R, T, self._stream())
        return self._graph_done(rc, 'qagnn_graph_from_blobs', storage, g, N, E, R, T, n, packed.e_cap is not None, packed.buf,
                                f'the blob batch with B={B} samples, E={packed.E} edges (edge endpoint / relation id / node type)')

    def _cstore(self, store):
        """the qagnn_store of a data_utils.DeviceGraphStore on the GPU (built once per store, kept on it)"""
        st = getattr(store, '_cstruct', None)
        if st is None:
            for t, dt in ((store.blobs, torch.int32), (store.blob_off, torch.long), (store.concept_ids, torch.long), (store.node_type_ids, torch.long),
                          (store.node_scores, torch.float32), (store.adj_lengths, torch.long)):
                assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == store.blobs.device
            assert store.blob_off.numel() == store.S + 1 and store.concept_ids.shape == (store.S, store.n) == store.node_type_ids.shape \
                and store.node_scores.shape == (store.S, store.n) and store.adj_lengths.shape == (store.S,)
            st = store._cstruct = qagnn_store(store.blobs.data_ptr(), store.blob_off.data_ptr(), store.concept_ids.data_ptr(),
                                              store.node_type_ids.data_ptr(), store.node_scores.data_ptr(), store.adj_lengths.data_ptr(),
                                              store.S, store.n, store.blobs.numel())
        return st

    def store_gather(self, store, ids):
        """store: data_utils.DeviceGraphStore on the GPU; ids: int32 device tensor [B] of sample ids.  -> (concept_ids [B, n] int64, node_type_ids
        [B, n] int64, node_scores [B, n] fp32, adj_lengths [B] int64, edge_off [B + 1] int32, flags [4] int32): the batch's rows of the store and
        the exclusive prefix sum of its samples' edge counts, one launch (qagnn_store_gather).  An id outside the store is clamped on the
        device and reported through ERR_WATCH."""
        assert ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous() and ids.device == store.blobs.device
        B, n, dev = ids.numel(), store.n, ids.device
        cids = torch.empty((B, n), dtype=torch.long, device=dev)
        nt = torch.empty((B, n), dtype=torch.long, device=dev)
        ns = torch.empty((B, n), dtype=torch.float32, device=dev)
        al = torch.empty((B,), dtype=torch.long, device=dev)
        edge_off = torch.empty((B + 1,), dtype=torch.int32, device=dev)
        flags = torch.zeros(4, dtype=torch.int32, device=dev)  # (a fresh flag per call, like node_prep's)
        rc = self.lib.qagnn_store_gather(C.byref(self._cstore(store)), ids.data_ptr(), B, cids.data_ptr(), nt.data_ptr(), ns.data_ptr(),
                                         al.data_ptr(), edge_off.data_ptr(), flags.data_ptr(), self._stream())
        self._check(rc, 'qagnn_store_gather')
        ERR_WATCH.poll()
        ERR_WATCH.watch(flags, f'the sample ids of a batch of {B} (an id outside the device store\'s {store.S} samples)')
        return cids, nt, ns, al, edge_off, flags

    def graph_from_store(self, batch, node_type):
        """batch: data_utils.StoreBatch on the GPU; node_type [B*n] int64, the batch's (batch.fields()[1]).  graph_from_blobs() with every
        sample's blob read where it lies in the device store (qagnn_graph_from_store); the edge offsets are those of the batch's gather.
        batch.e_cap (optional, >= batch.E): the edge capacity, as PackedGraphBatch.e_cap."""
        assert node_type.is_cuda and node_type.dtype == torch.long and node_type.is_contiguous()
        store, B, n, R, T = batch.dstore, batch.B, batch.n, batch.n_etype, batch.n_ntype
        edge_off = batch.gathered()[4]
        E = batch.E if batch.e_cap is None else int(batch.e_cap)
        assert E >= batch.E, f'edge capacity {E} below the batch\'s {batch.E} edges'
        N = B * n
        assert node_type.numel() == N and batch.ids.numel() == B and edge_off.numel() == B + 1
        storage, g = self._graph_alloc(N, E, R, T, node_type.device)
        rc = self.lib.qagnn_graph_from_store(C.byref(g), storage.data_ptr(), C.byref(self._cstore(store)), batch.ids.data_ptr(), edge_off.data_ptr(),
                                             node_type.data_ptr(), B, E, R, T, self._stream())
        return self._graph_done(rc, 'qagnn_graph_from_store', storage, g, N, E, R, T, n, batch.e_cap is not None, (store, batch.ids, edge_off),
                                f'the store batch with B={B} samples, E={batch.E} edges (sample id / blob field / node type)')

    def seed_epoch_advance(self, delta=1):
        """Advance this device's dropout seed epoch (see qagnn_seed_epoch_advance): the last launch of a captured training step."""
        self._check(self.lib.qagnn_seed_epoch_advance(int(delta), self._stream()), 'qagnn_seed_epoch_advance')

    def seed_epoch_set(self, value=0):
        self._check(self.lib.qagnn_seed_epoch_set(int(value), self._stream()), 'qagnn_seed_epoch_set')

    def node_prep(self, node_scores, adj_lengths, node_type_ids, concept_ids, table_rows=0):
        """-> (normalised scores [B, n] fp32, pooling mask [B, n] bool, entity-table row ids [B*n] int64); qagnn_node_prep_f32.
        table_rows > 0: concept ids outside the entity table become the zero row and are reported through ERR_WATCH (the
        reference's nn.Embedding raises on them)."""
        B, n = node_type_ids.shape
        raw = node_scores.reshape(B, n).float().contiguous()  # the reference computes the normalisation in fp32 (qagnn.py: fp32 inputs)
        assert raw.dtype == torch.float32 and raw.is_contiguous() and adj_lengths.dtype == torch.long and adj_lengths.is_contiguous()
        assert node_type_ids.dtype == torch.long and node_type_ids.is_contiguous() and concept_ids.dtype == torch.long and concept_ids.is_contiguous()
        dev = node_type_ids.device
        score = torch.empty((B, n), dtype=torch.float32, device=dev)
        mask = torch.empty((B, n), dtype=torch.bool, device=dev)
        ridx = torch.empty(B * n, dtype=torch.long, device=dev)
        # a fresh flag per call, like graph_prep's err words: a persistent one would still read 1 in the batch AFTER a bad id
        flags = torch.zeros(4, dtype=torch.int32, device=dev) if table_rows > 0 else None
        rc = self.lib.qagnn_node_prep_f32(raw.data_ptr(), adj_lengths.data_ptr(), node_type_ids.data_ptr(), concept_ids.data_ptr(), B, n,
                                          score.data_ptr(), mask.data_ptr(), ridx.data_ptr(), int(table_rows), _ptr(flags), self._stream())
        self._check(rc, 'qagnn_node_prep_f32')
        if flags is not None:
            ERR_WATCH.poll()
            ERR_WATCH.watch(flags, 'concept_ids (an id outside the entity table)')
        return score, mask, ridx

    def radam_step(self, params, grads, exp_avgs, exp_avg_sqs, beta1, beta2, eps, lr, weight_decay, step_size, mode, grad_scale=None):
        """One fused RAdam update of a list of fp32 device tensors that share a step count (qagnn_radam_step_f32).
        grad_scale: a one-element fp32 device tensor (grad_norm()'s coefficient word) every gradient is multiplied by as it is read
        (qagnn_radam_step_scaled_f32); the gradients are not written."""
        n = len(params)
        for group in (params, grads, exp_avgs, exp_avg_sqs):
            assert len(group) == n and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in group)
        assert all(p.numel() == g.numel() == m.numel() == v.numel() for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs))
        tab = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        numel = (C.c_int64 * n)(*[t.numel() for t in params])
        args = (n, tab(params), tab(grads), tab(exp_avgs), tab(exp_avg_sqs), numel, float(beta1), float(beta2),
                float(eps), float(lr), float(weight_decay), float(step_size), int(mode))
        if grad_scale is None:
            self._check(self.lib.qagnn_radam_step_f32(*args, self._stream()), 'qagnn_radam_step_f32')
            return
        self._check_scale_word(grad_scale, params[0].device if n else grad_scale.device)
        self._check(self.lib.qagnn_radam_step_scaled_f32(*args, grad_scale.data_ptr(), self._stream()), 'qagnn_radam_step_scaled_f32')

    GRAD_NORM_CHUNK, GRAD_NORM_THREADS = 4096, 256  # csrc/optim.hip: MT_CHUNK, MT_THREADS (the reduction shape of grad_norm's stage 1)

    @staticmethod
    def _check_scale_word(scale, device):
        assert scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1 and scale.device == device, \
            f'need a one-element fp32 tensor on {device}, got {tuple(scale.shape)} {scale.dtype} {scale.device}'

    @staticmethod
    def _grad_table(grads):
        n = len(grads)
        assert all(g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.device == grads[0].device for g in grads)
        return n, (C.c_void_p * n)(*[g.data_ptr() for g in grads]), (C.c_int64 * n)(*[g.numel() for g in grads])

    def grad_norm(self, grads, max_norm, workspace=None):
        """-> fp32 [2] on the gradients' device: [0] the global L2 norm of a list of fp32 device tensors, [1] the clip coefficient
        min(1, max_norm / (norm + 1e-6)) (qagnn_grad_norm_f32; torch.nn.utils.clip_grad_norm_'s formula).  Nothing comes back to the host.
        workspace: an fp32 device tensor of at least grad_norm_workspace_elems(grads) elements (else one is allocated)."""
        n, tab, numel = self._grad_table(grads)
        dev = grads[0].device if n else torch.device('cuda', torch.cuda.current_device())
        need = int(self.lib.qagnn_grad_norm_workspace_elems(n, numel))
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.float32, device=dev)
        assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.device == dev \
            and workspace.numel() >= need, f'grad_norm: need {need} fp32 workspace elements on {dev}'
        out = torch.empty(2, dtype=torch.float32, device=dev)
        self._check(self.lib.qagnn_grad_norm_f32(n, tab, numel, float(max_norm), workspace.data_ptr(), out.data_ptr(), self._stream()),
                    'qagnn_grad_norm_f32')
        return out

    def grad_norm_workspace_elems(self, grads):
        n, _, numel = self._grad_table(grads)
        return int(self.lib.qagnn_grad_norm_workspace_elems(n, numel))

    def scale_multi(self, grads, scale):
        """g *= scale[0] for every tensor of a list of fp32 device tensors, scale a one-element device tensor (qagnn_scale_multi_f32)."""
        n, tab, numel = self._grad_table(grads)
        if n == 0:
            return
        self._check_scale_word(scale, grads[0].device)
        self._check(self.lib.qagnn_scale_multi_f32(n, tab, numel, scale.data_ptr(), self._stream()), 'qagnn_scale_multi_f32')

    # -- GEMMs ---------------------------------------------------------------------------------------------------
    STAT_TILE = 128  # rows per tile of the column statistics a GEMM can leave behind (gemm_split.hip: SBM)

    def colstats_supported(self, M, K1, No):
        """Can gemm_nn(..., colstats=True) deliver per-tile column statistics for this shape?  (the bf16-split kernel, 193..208 columns)"""
        return self.gemm_split and 192 < No <= 208 and K1 % 4 == 0 and M * max(K1, No) * 4 < 2 ** 31 - 1

    def prepack(self, pairs, tag):
        """Pack the B operands of the coming large NN products in ONE launch (qagnn_gemm_nn_prepack_f32) and register them under `tag`:
        pairs = [(B1n, B2n or None), ...], each weight in its [No, K] layout exactly as gemm_nn() will receive it.  Returns what must
        stay alive (and unchanged) until the tag is cleared or packed again: the packed buffer and the weights themselves."""
        descs = (qagnn_pack_desc * len(pairs))()
        for d, pr in zip(descs, pairs):
            b1, b2 = pr[0], pr[1]
            d.pieces = pr[2] if len(pr) > 2 else 3  # (b1, b2, 2): the two scaled fp16 images of the three-MFMA form
            _chkp(b1, 'B1n')
            d.B1n, d.ldn1, d.K1, d.No = b1.data_ptr(), _ld(b1), b1.size(1), b1.size(0)
            if b2 is not None:
                _chkp(b2, 'B2n')
                assert b2.size(0) == b1.size(0)
                d.B2n, d.ldn2, d.K2 = b2.data_ptr(), _ld(b2), b2.size(1)
        nbytes = self.lib.qagnn_gemm_nn_prepack_bytes(descs, len(pairs))
        out = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=pairs[0][0].device)
        self._check(self.lib.qagnn_gemm_nn_prepack_f32(descs, len(pairs), out.data_ptr(), out.numel(), int(tag), self._stream()),
                    'qagnn_gemm_nn_prepack_f32')
        # (detached aliases: they pin the storage, not the autograd graph that produced the weights -- a kept-alive graph of the previous
        # iteration makes its AccumulateGrad nodes run on THEIR stream during a later hipGraph capture, which breaks the capture)
        return out, [t.detach() for pr in pairs for t in pr[:2] if t is not None]

    def prepack_clear(self, tag=0):
        self.lib.qagnn_gemm_nn_prepack_clear(int(tag))

    def gemm_nn(self, A1, B1, A2=None, B2=None, bias=None, rowtab=None, rowidx=None, a_scale=None, a_shift=None,
                out=None, accumulate=False, a_rowidx=None, B1n=None, B2n=None, colstats=False, a_amax1=None, a_amax2=None):
        """B1n / B2n: the same weights as B1 / B2 in their [No, K] layout (optional); with them the product runs on the bf16 matrix
        cores by exact operand splitting (see gemm_split.hip), else on the fp32-input MFMAs.
        colstats=True (only where colstats_supported()): returns (C, part) with part [ceil(M/128), 3, No] = per 128-row tile x0 | S1 | S2
        of C's columns, for bn_stats_finalize."""
        _chkp(A1, 'A1'), _chkp(B1, 'B1')
        K1 = A1.size(1)
        M = A1.size(0) if a_rowidx is None else a_rowidx.numel()
        No = B1.size(1)
        assert B1.size(0) == K1
        a = qagnn_gemm_nn_args()
        a.A1, a.lda1, a.K1, a.B1, a.ldb1 = A1.data_ptr(), _ld(A1), K1, B1.data_ptr(), _ld(B1)
        if A2 is not None:
            _chkp(A2, 'A2'), _chkp(B2, 'B2')
            assert A2.size(0) == M and B2.shape == (A2.size(1), No)
            a.A2, a.lda2, a.K2, a.B2, a.ldb2 = A2.data_ptr(), _ld(A2), A2.size(1), B2.data_ptr(), _ld(B2)
        if out is None:
            assert not accumulate
            out = torch.empty((M, No), dtype=torch.float32, device=A1.device)
        else:
            _chkp(out, 'out')
            assert out.shape == (M, No)
        a.C, a.ldc, a.M, a.No = out.data_ptr(), _ld(out), M, No
        if bias is not None:
            assert bias.is_contiguous() and bias.numel() == No and bias.dtype == torch.float32
            a.bias = bias.data_ptr()
        if rowtab is not None:
            _chkp(rowtab, 'rowtab')
            assert rowtab.size(1) == No and rowidx.dtype == torch.long and rowidx.numel() == M and rowidx.is_contiguous()
            a.rowtab, a.ldt, a.rowidx = rowtab.data_ptr(), _ld(rowtab), rowidx.data_ptr()
        if a_scale is not None:
            assert a_scale.numel() == K1 and a_shift.numel() == K1 and a_scale.is_contiguous() and a_shift.is_contiguous()
            a.a_scale, a.a_shift = a_scale.data_ptr(), a_shift.data_ptr()
        a.accumulate = 1 if accumulate else 0
        if a_amax1 is not None and self.gemm_split >= 2:  # int32 [1] device words: absmax() of A1 / A2 -> the three-MFMA form
            assert a_amax1.dtype == torch.int32 and a_amax1.is_cuda and (A2 is None or a_amax2 is not None)
            a.a_amax1, a.a_amax2 = a_amax1.data_ptr(), _ptr(a_amax2)
            a.pieces = 1 if self.gemm_split == 3 else 0  # (3: the reduced-precision form, on request only)
        if a_rowidx is not None:
            assert a_rowidx.dtype == torch.long and a_rowidx.is_contiguous() and a_rowidx.is_cuda
            a.a_rowidx = a_rowidx.data_ptr()
            a.a_rows = A1.size(0)  # (the table's extent: lets the gathered product take the second-generation kernels)
        part = None
        if colstats:
            assert self.colstats_supported(M, K1, No) and B1n is not None and A2 is None and rowtab is None and a_scale is None and a_rowidx is None \
                and not accumulate, 'gemm_nn(colstats=True): bias-only epilogue on the split kernel'
            part = torch.empty((-(-M // self.STAT_TILE), 3, No), dtype=torch.float32, device=A1.device)
            a.colstat_part = part.data_ptr()
        if self.gemm_split and B1n is not None and (A2 is None or B2n is not None) and K1 % 4 == 0 and (A2 is None or A2.size(1) % 4 == 0):
            _chkp(B1n, 'B1n')
            assert B1n.shape == (No, K1)
            n2, ld1, ld2 = None, _ld(B1n), 0
            if A2 is not None:
                _chkp(B2n, 'B2n')
                assert B2n.shape == (No, A2.size(1))
                n2, ld2 = B2n.data_ptr(), _ld(B2n)
            # large products whose B is not registered (qagnn_gemm_nn_prepack_f32): B is split ONCE into the kernel's LDS image order
            # (scratch from the caching allocator, stream-ordered: the next product may reuse it), every row tile then streams it by DMA
            # instead of repeating the split.  The library says whether this very call would use the scratch (0: pre-packed / not taken)
            ws_bytes = self.lib.qagnn_gemm_nn_ws_bytes(C.byref(a), B1n.data_ptr(), ld1, n2, ld2) if M >= self.PACK_MIN_M else 0
            if ws_bytes > 0:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=A1.device)
                self._check(self.lib.qagnn_gemm_nn_split_ws_f32(C.byref(a), B1n.data_ptr(), ld1, n2, ld2, ws.data_ptr(), ws_bytes, self._stream()),
                            'qagnn_gemm_nn_split_ws_f32')
            else:
                self._check(self.lib.qagnn_gemm_nn_split_f32(C.byref(a), B1n.data_ptr(), ld1, n2, ld2, self._stream()), 'qagnn_gemm_nn_split_f32')
            return (out, part) if colstats else out
        assert K1 % 16 == 0 and (A2 is None or A2.size(1) % 16 == 0), 'the fp32-MFMA kernel needs K to be a multiple of 16'
        self._check(self.lib.qagnn_gemm_nn_f32(C.byref(a), self._stream()), 'qagnn_gemm_nn_f32')
        return out

    def _tn_out_ws(self, R, Ka, No, out, dev):
        """the [Ka, No] output of a weight-gradient product over R rows (the caller's `out`, or a fresh one) and its split-K workspace"""
        if out is None:
            out = torch.empty((Ka, No), dtype=torch.float32, device=dev)
        else:
            _chkp(out, 'out')
            assert out.shape == (Ka, No)
        return out, torch.empty(self.lib.qagnn_gemm_tn_workspace_elems(R, Ka, No), dtype=torch.float32, device=dev)

    def gemm_tn(self, A, B, a_scale=None, a_shift=None, out=None, accumulate=False, a_rowidx=None, colsum_groups=0,
                b_rowidx=None):
        """C = A^T B.  colsum_groups = G > 0 additionally returns bsum [G, No] = per-group column sums of B."""
        _chkp(A, 'A'), _chkp(B, 'B')
        Ka = A.size(1)
        R, No = B.shape
        assert (A.size(0) == R) if a_rowidx is None else (a_rowidx.numel() == R and a_rowidx.dtype == torch.long)
        assert out is not None or not accumulate
        out, ws = self._tn_out_ws(R, Ka, No, out, A.device)
        bsum = None
        if colsum_groups:
            assert b_rowidx is None or (b_rowidx.dtype == torch.long and b_rowidx.numel() == R and b_rowidx.is_contiguous())
            bsum = torch.empty((colsum_groups, No), dtype=torch.float32, device=A.device)
        rc = self.lib.qagnn_gemm_tn_colsum_f32(A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), out.data_ptr(), _ld(out), R, Ka, No, _ptr(a_scale),
                                               _ptr(a_shift), _ptr(a_rowidx), 1 if accumulate else 0, _ptr(bsum), _ptr(b_rowidx),
                                               colsum_groups, ws.data_ptr(), self._stream())
        self._check(rc, 'qagnn_gemm_tn_colsum_f32')
        return (out, bsum) if colsum_groups else out

    def absmax(self, x, out=None):
        """int32 [1]: the bit pattern of max |x| (qagnn_absmax_f32 into a zeroed word) -- the operand maximum of the three-MFMA GEMM form"""
        assert x.is_contiguous() and x.dtype == torch.float32 and x.numel() % 4 == 0
        if out is None:
            out = torch.empty(4, dtype=torch.int32, device=x.device)
            self._check(self.lib.qagnn_zero_words(out.data_ptr(), 4, self._stream()), 'qagnn_zero_words')
        self._check(self.lib.qagnn_absmax_f32(x.data_ptr(), x.numel(), out.data_ptr(), self._stream()), 'qagnn_absmax_f32')
        return out

    def gemm_tn_h2(self, A1, B, amax_a1, amax_b, A2=None, amax_a2=None, a_scale=None, a_shift=None, out=None):
        """[A1 | A2]^T B in the three-MFMA form (qagnn_gemm_tn_h2_f32); amax_*: absmax() words (amax_a1 AFTER the scale / shift prologue)"""
        _chkp(A1, 'A1'), _chkp(B, 'B')
        if A2 is not None:
            _chkp(A2, 'A2')
        Ka1, Ka2 = A1.size(1), (A2.size(1) if A2 is not None else 0)
        R, No = B.shape
        out, ws = self._tn_out_ws(R, Ka1 + Ka2, No, out, B.device)
        fn = self.lib.qagnn_gemm_tn_h1_f32 if self.gemm_split == 3 else self.lib.qagnn_gemm_tn_h2_f32
        rc = fn(A1.data_ptr(), _ld(A1), Ka1, _ptr(A2), _ld(A2) if A2 is not None else 0, Ka2, B.data_ptr(), _ld(B), out.data_ptr(), _ld(out), R, No, _ptr(a_scale),
                                           _ptr(a_shift), amax_a1.data_ptr(), _ptr(amax_a2), amax_b.data_ptr(), ws.data_ptr(), self._stream())
        self._check(rc, 'qagnn_gemm_tn_h2_f32')
        return out

    def gemm_tn_graph(self, A1, A2, B, graph=None, pieces=3, amax=None, out=None):
        """[A1 | A2]^T B for a B = dK | dM | dQ over the node rows of `graph` (qagnn_gemm_tn_graph_f32): the K / Q columns skip the graph's dead
        k-tiles where the dispatch runs the long two-operand kernel.  graph=None: the plain product.  pieces 3 | 2 | 1; amax = (a1, a2, b)
        absmax() words for pieces < 3."""
        _chkp(A1, 'A1'), _chkp(A2, 'A2'), _chkp(B, 'B')
        Ka1, Ka2 = A1.size(1), A2.size(1)
        R, No = B.shape
        assert A1.size(0) == R and A2.size(0) == R and (pieces == 3 or amax is not None)
        out, ws = self._tn_out_ws(R, Ka1 + Ka2, No, out, B.device)
        am = [None, None, None] if amax is None else [t.data_ptr() for t in amax]
        rc = self.lib.qagnn_gemm_tn_graph_f32(A1.data_ptr(), _ld(A1), Ka1, A2.data_ptr(), _ld(A2), Ka2, B.data_ptr(), _ld(B), out.data_ptr(), _ld(out),
                                              R, No, am[0], am[1], am[2], pieces, C.byref(graph.c) if graph is not None else None, ws.data_ptr(),
                                              self._stream())
        self._check(rc, 'qagnn_gemm_tn_graph_f32')
        return out

    def gemm_nn_dual(self, A, B1n, B2n, a_amax, out1, out2, accumulate1=False, accumulate2=False, ws=None):
        """out1 (+)= A B1n^T and out2 (+)= A B2n^T in ONE launch (qagnn_gemm_nn_dual_f32: bit-identical to the two gemm_nn calls).  B1n / B2n:
        the weights as [No, K]; a_amax: the absmax() word of A.  ws: the caller's uint8 scratch for the images that are not registered
        (qagnn_gemm_nn_pack_bytes(624, 208, 208) holds both), or None.  Returns the status (0, or QAGNN_EUNSUPPORTED = 2 when the pair is
        not one the launch takes: nothing was enqueued); other errors raise."""
        for t, n in ((A, 'A'), (B1n, 'B1n'), (B2n, 'B2n'), (out1, 'out1'), (out2, 'out2')):
            _chkp(t, n)
        assert ws is None or (ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous())
        a1, a2 = dual_args(A.data_ptr(), _ld(A), A.size(0), A.size(1), _ptr(a_amax), out1.data_ptr(), _ld(out1), B1n.size(0),
                           out2.data_ptr(), _ld(out2), B2n.size(0), accumulate1, accumulate2)
        rc = self.lib.qagnn_gemm_nn_dual_f32(C.byref(a1), B1n.data_ptr(), _ld(B1n), C.byref(a2), B2n.data_ptr(), _ld(B2n),
                                             _ptr(ws), ws.numel() if ws is not None else 0, self._stream())
        if rc != 2:
            self._check(rc, 'qagnn_gemm_nn_dual_f32')
        return rc

    def nn_dual_enable(self, on):
        """TESTS AND A/B RUNS ONLY: the process-wide mode of the two-output dX / dS launch (qagnn_nn_dual_enable): 0 off, 1 where the separate
        launches would keep their full column tiles, 2 at every row count of the packed forms; -1 reads.  Returns the previous value."""
        return int(self.lib.qagnn_nn_dual_enable(int(on)))

    def dual_launches(self):
        """launches of the two-output kernel since the library was loaded (qagnn_dual_launches)"""
        return int(self.lib.qagnn_dual_launches())

    def tn_route_query(self, R, Ka1, Ka2, No):
        """host-only: (family, chunk_rows, nchunks, live) of the weight gradient [A1 | A2]^T B (qagnn_gemm_tn_route_query); family 3 = k_gemm_tn_ws"""
        out = (C.c_int32 * 4)()
        self._check(self.lib.qagnn_gemm_tn_route_query(R, Ka1, Ka2, No, C.cast(out, C.c_void_p)), 'qagnn_gemm_tn_route_query')
        return tuple(out)

    def tn_work_table(self, graph, S, chunk_tiles):
        """int32 [4 + 5 S]: cK, cM, T, L, then (column block, list?, first, tiles, partial tile) per unit (qagnn_tn_work_table)"""
        out = torch.empty(4 + 5 * S, dtype=torch.int32, device=graph.storage.device)
        self._check(self.lib.qagnn_tn_work_table(C.byref(graph.c), S, chunk_tiles, out.data_ptr(), self._stream()), 'qagnn_tn_work_table')
        return out

    def tn_live_tiles(self, on):
        """TESTS AND A/B RUNS ONLY: the process-wide switch of the live-tile weight gradient (-1 reads); returns the previous value"""
        return int(self.lib.qagnn_tn_live_tiles(int(on)))

    def gemm_tn2(self, A1, A2, B, out=None):
        """[A1 | A2]^T B -> [Ka1 + Ka2, No]: two weight gradients that share their B operand, one launch (qagnn_gemm_tn2_f32)."""
        _chkp(A1, 'A1'), _chkp(A2, 'A2'), _chkp(B, 'B')
        Ka1, Ka2 = A1.size(1), A2.size(1)
        R, No = B.shape
        assert A1.size(0) == R and A2.size(0) == R
        out, ws = self._tn_out_ws(R, Ka1 + Ka2, No, out, B.device)
        rc = self.lib.qagnn_gemm_tn2_f32(A1.data_ptr(), _ld(A1), Ka1, A2.data_ptr(), _ld(A2), Ka2, B.data_ptr(), _ld(B), out.data_ptr(), _ld(out), R, No,
                                         ws.data_ptr(), self._stream())
        self._check(rc, 'qagnn_gemm_tn2_f32')
        return out

    # -- reductions / elementwise ----------------------------------------------------------------------------------
    def _colreduce(self, mode, X, X2, rowidx, groups, mean, invstd, scale, shift, nout, out_scale=1.0, roww=None, out=None):
        _chkp(X, 'X')
        R, Cc = X.shape
        if out is None:
            out = torch.empty((nout, Cc), dtype=torch.float32, device=X.device)
        else:
            assert out.shape == (nout, Cc) and out.is_contiguous() and out.dtype == torch.float32
        ws = torch.empty(self.lib.qagnn_colreduce_workspace_elems(R, Cc, groups), dtype=torch.float32, device=X.device)
        rc = self.lib.qagnn_colreduce_f32(mode, X.data_ptr(), _ld(X), _ptr(X2), _ld(X2) if X2 is not None else Cc, R, Cc, _ptr(rowidx), groups, _ptr(mean),
                                          _ptr(invstd), _ptr(scale), _ptr(shift), _ptr(roww), float(out_scale), out.data_ptr(), ws.data_ptr(), self._stream())
        self._check(rc, 'qagnn_colreduce_f32')
        return out

    def colsum(self, X, rowidx=None, groups=1, scale=1.0, roww=None, out=None):
        return self._colreduce(0, X, None, rowidx, groups, None, None, None, None, groups, scale, roww, out=out)

    def colvar_sum(self, X, mean, scale=1.0, roww=None):
        return self._colreduce(1, X, None, None, 1, mean, None, None, None, 1, scale, roww)[0]

    def bn_finalize(self, mean, var, gamma, beta, eps, running=None, ones_col=-1):
        """-> invstd, scale, shift [Cc]; running = (run_mean [d], run_var [d], num_batches_tracked, dense_pos [d], momentum, unbias)
        additionally applies the train-mode running-statistics update in the same launch.  ones_col >= 0: that (padding) column gets
        scale 0 / shift 1, i.e. relu(bn(h)) carries a column of ones there (see qagnn_bn_finalize_f32)."""
        Cc = mean.numel()
        out = torch.empty((3, Cc), dtype=torch.float32, device=mean.device)
        rc = self.lib.qagnn_bn_finalize_f32(mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps),
                                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), Cc, *_running_fields(running),
                                            int(ones_col), self._stream())
        self._check(rc, 'qagnn_bn_finalize_f32')
        return out[0], out[1], out[2]

    def bn_stats_finalize(self, part, rows, gamma, beta, eps, running=None, ones_col=-1):
        """part: what gemm_nn(colstats=True) returned for the [rows, Cc] BatchNorm input -> stats [5, Cc] = mean | biased var | invstd |
        scale | shift, plus (running given) the train-mode running-statistics update: qagnn_bn_stats_finalize_f32, one launch."""
        nt, _, Cc = part.shape
        assert part.is_contiguous() and nt == -(-rows // self.STAT_TILE)
        stats = torch.empty((5, Cc), dtype=torch.float32, device=part.device)
        rc = self.lib.qagnn_bn_stats_finalize_f32(part.data_ptr(), nt, int(rows), Cc, gamma.data_ptr(), beta.data_ptr(), float(eps), stats.data_ptr(),
                                                  *_running_fields(running), int(ones_col), self._stream())
        self._check(rc, 'qagnn_bn_stats_finalize_f32')
        return stats

    def bn_bwd_reduce(self, dR, H, mean, invstd, scale, shift):
        _chkp(H, 'H')
        assert H.shape == dR.shape
        return self._colreduce(2, dR, H, None, 1, mean, invstd, scale, shift, 2)

    @staticmethod
    def _bn_bwd_operands(dR, H, dH):
        """dR, H and dH [R, Cc] share ONE row pitch (the entry points take a single ld) -> (dH, ld); dH=None: a fresh contiguous one,
        which asks dR and H to be contiguous too"""
        _chkp(dR, 'dR'), _chkp(H, 'H')
        if dH is None:
            dH = torch.empty(H.shape, dtype=torch.float32, device=H.device)
        _chkp(dH, 'dH')
        assert dR.shape == H.shape == dH.shape and _ld(dR) == _ld(H) == _ld(dH), \
            f'bn_relu_bwd: dR, H and dH share one row pitch, got {_ld(dR)}, {_ld(H)}, {_ld(dH)}'
        return dH, _ld(H)

    def bn_relu_bwd(self, dR, H, mean, invstd, scale, shift, gamma, red, inv_rows, roww=None, dH=None):
        """red = bn_bwd_reduce(...) [2, Cc]; inv_rows = 1/R (batch statistics) or 0 (running statistics); roww [R]: the
        per-row statistics weights when they were not uniform.  dH: the output, a view with the pitch of dR and H (else allocated)."""
        assert red.is_contiguous() and red.shape == (2, H.size(1))
        dH, ld = self._bn_bwd_operands(dR, H, dH)
        R, Cc = H.shape
        rc = self.lib.qagnn_bn_relu_bwd_f32(dR.data_ptr(), H.data_ptr(), dH.data_ptr(), ld, R, Cc, mean.data_ptr(),
                                            invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), gamma.data_ptr(),
                                            red[0].data_ptr(), red[1].data_ptr(), float(inv_rows), _ptr(roww), self._stream())
        self._check(rc, 'qagnn_bn_relu_bwd_f32')
        return dH

    POOL_LIMITS = (4, 256, 1024)  # heads, row width, nodes per subgraph

    def pool_attn_fwd(self, u, cvec, K, mask, inv_temp, p, seed):
        """u [B, NH, Cc], cvec [B, NH], K [B, n, Cc] (rows with one pitch >= Cc), mask [B, n] bool -> attn, attn_d [B, NH, n], z [B, NH, Cc]."""
        B, NH, Cc = u.shape
        n = K.size(1)
        assert u.is_contiguous() and cvec.is_contiguous() and mask.is_contiguous() and mask.dtype == torch.bool
        _chkp3(K, 'K')
        attn = torch.empty((2, B, NH, n), dtype=torch.float32, device=u.device)
        z = torch.empty((B, NH, Cc), dtype=torch.float32, device=u.device)
        rc = self.lib.qagnn_pool_attn_fwd_f32(u.data_ptr(), cvec.data_ptr(), K.data_ptr(), _ld3(K), mask.data_ptr(), B, n, NH, Cc,
                                              float(inv_temp), float(p), int(seed), attn[0].data_ptr(), attn[1].data_ptr(),
                                              z.data_ptr(), self._stream())
        self._check(rc, 'qagnn_pool_attn_fwd_f32')
        return attn[0], attn[1], z

    def pool_attn_bwd(self, u, K, inv_temp, p, seed, attn, attn_d, dz, dattn_d, dK=None):
        """dK: the [B, n, Cc] output, rows with a pitch of its own (else a contiguous one is allocated)"""
        B, NH, Cc = u.shape
        n = K.size(1)
        assert dz.is_contiguous() and attn.is_contiguous() and attn_d.is_contiguous() and (dattn_d is None or dattn_d.is_contiguous())
        _chkp3(K, 'K')
        if dK is None:
            dK = torch.empty(K.shape, dtype=torch.float32, device=K.device)
        assert _chkp3(dK, 'dK').shape == K.shape
        du = torch.empty_like(u)
        dc = torch.empty((B, NH), dtype=torch.float32, device=u.device)
        rc = self.lib.qagnn_pool_attn_bwd_f32(u.data_ptr(), K.data_ptr(), _ld3(K), B, n, NH, Cc, float(inv_temp), float(p), int(seed),
                                              attn.data_ptr(), attn_d.data_ptr(), dz.data_ptr(), _ptr(dattn_d), dK.data_ptr(), _ld3(dK), du.data_ptr(),
                                              dc.data_ptr(), self._stream())
        self._check(rc, 'qagnn_pool_attn_bwd_f32')
        return dK, du, dc

    HEAD_LIMITS = (4, 256, 256)  # heads, NH * dv, DP of qagnn_head_post_{fwd,bwd}_f32

    def head_post_fwd(self, z, attn, BDv, bv, sent, K3, d, w_fc, b_fc, p_pool, p_fc, seed_pool, seed_fc):
        """z [B, NH, DP], attn [B, NH, n] (after dropout), BDv [NH*DP, NH*dv], bv [NH*dv], sent [B, Ds], K3 [B, n, DP] (row 0 of every
        subgraph is read), w_fc [NH*dv + Ds + d], b_fc [1] -> logits [B], out [B, NH*dv] (before dropout), asum [B, NH]."""
        B, NH, DP = z.shape
        n, NO, Ds = attn.size(2), BDv.size(1), sent.size(1)
        for t in (z, attn, BDv, bv, sent, w_fc, b_fc):
            assert t.is_contiguous() and t.dtype == torch.float32
        assert _chkp3(K3, 'K3').shape == (B, n, DP) and BDv.size(0) == NH * DP and NO % NH == 0 and w_fc.numel() == NO + Ds + d and sent.size(0) == B
        out = torch.empty((B, NO), dtype=torch.float32, device=z.device)
        asum = torch.empty((B, NH), dtype=torch.float32, device=z.device)
        logits = torch.empty((B,), dtype=torch.float32, device=z.device)
        rc = self.lib.qagnn_head_post_fwd_f32(z.data_ptr(), attn.data_ptr(), BDv.data_ptr(), bv.data_ptr(), sent.data_ptr(), K3.data_ptr(), n * _ld3(K3),
                                              w_fc.data_ptr(), b_fc.data_ptr(), B, NH, DP, NO // NH, n, Ds, d, float(p_pool), float(p_fc),
                                              int(seed_pool), int(seed_fc), out.data_ptr(), asum.data_ptr(), logits.data_ptr(), self._stream())
        self._check(rc, 'qagnn_head_post_fwd_f32')
        return logits, out, asum

    def head_post_bwd(self, dlogits, out, asum, BDv, bv, sent, K3, d, w_fc, p_pool, p_fc, seed_pool, seed_fc, n, need_dsent, ldp=None, part=None):
        """-> dz [B, NH, DP], dattn [B, NH, n], dout [B, NH*dv], dsent [B, Ds] or None, dZ [B, DP], part [B, ldp] (L + NH*dv + 1 <= ldp <=
        L + NH*dv + 1 + 255, a multiple of 4; default the smallest: the columns past L + NH*dv + 1 are zero, and one pass of the kernel's
        256 threads zeroes them, hence the upper limit).  part: the caller's [B, ldp] buffer (every column of its rows is written)"""
        B, NO = out.shape
        NH, DP, Ds = asum.size(1), K3.size(2), sent.size(1)
        assert dlogits.is_contiguous() and dlogits.numel() == B
        _chkp3(K3, 'K3')
        ldp_min = (NO + Ds + d + NO + 1 + 3) // 4 * 4  # (pitch: a multiple of 4 for the column sums)
        ldp = (ldp_min if part is None else part.size(1)) if ldp is None else int(ldp)
        assert ldp_min <= ldp <= NO + Ds + d + NO + 1 + 255 and ldp % 4 == 0, f'ldp={ldp}: a multiple of 4 in [{ldp_min}, {NO + Ds + d + NO + 1 + 255}]'
        dev = out.device
        dz = torch.empty((B, NH, DP), dtype=torch.float32, device=dev)
        dattn = torch.empty((B, NH, n), dtype=torch.float32, device=dev)
        dout = torch.empty((B, NO), dtype=torch.float32, device=dev)
        dsent = torch.empty((B, Ds), dtype=torch.float32, device=dev) if need_dsent else None
        dZ = torch.empty((B, DP), dtype=torch.float32, device=dev)
        if part is None:
            part = torch.empty((B, ldp), dtype=torch.float32, device=dev)
        assert part.is_cuda and part.dtype == torch.float32 and part.shape == (B, ldp) and part.is_contiguous()
        rc = self.lib.qagnn_head_post_bwd_f32(dlogits.data_ptr(), out.data_ptr(), asum.data_ptr(), BDv.data_ptr(), bv.data_ptr(), sent.data_ptr(),
                                              K3.data_ptr(), n * _ld3(K3), w_fc.data_ptr(), B, NH, DP, NO // NH, n, Ds, d, float(p_pool), float(p_fc),
                                              int(seed_pool), int(seed_fc), dz.data_ptr(), dattn.data_ptr(), dout.data_ptr(), _ptr(dsent),
                                              dZ.data_ptr(), part.data_ptr(), part.size(1), self._stream())
        self._check(rc, 'qagnn_head_post_bwd_f32')
        return dz, dattn, dout, dsent, dZ, part

    GATHER_MAX = GATHER_MAX

    @staticmethod
    def _gather_tabs(tensors):
        t = qagnn_gather_tabs()
        t.n = len(tensors)
        for i, x in enumerate(tensors):
            if x is not None:
                assert x.is_contiguous() and x.dtype == torch.float32
                t.p[i] = x.data_ptr()
        return t

    def gather_multi(self, sources, tid, off):
        """out[i] = sources[tid[i]].flat[off[i]] (tid < 0: 0); tid / off int32 on the device"""
        assert tid.dtype == torch.int32 and off.dtype == torch.int32 and tid.is_contiguous() and off.is_contiguous() and len(sources) <= GATHER_MAX
        out = torch.empty(tid.numel(), dtype=torch.float32, device=tid.device)
        t = self._gather_tabs(sources)
        self._check(self.lib.qagnn_gather_multi_f32(C.byref(t), tid.data_ptr(), off.data_ptr(), out.data_ptr(), tid.numel(), self._stream()),
                    'qagnn_gather_multi_f32')
        return out

    def gather_multi_sum(self, grads, tid, off):
        """out[s] = sum_k grads[tid[k, s]].flat[off[k, s]] (tid < 0 or an absent gradient: 0); tid / off [K, S] int32"""
        assert tid.dtype == torch.int32 and off.dtype == torch.int32 and tid.is_contiguous() and off.is_contiguous() and tid.dim() == 2
        assert len(grads) <= GATHER_MAX
        out = torch.empty(tid.size(1), dtype=torch.float32, device=tid.device)
        t = self._gather_tabs(grads)
        self._check(self.lib.qagnn_gather_multi_sum_f32(C.byref(t), tid.data_ptr(), off.data_ptr(), tid.size(0), tid.size(1), out.data_ptr(),
                                                        self._stream()), 'qagnn_gather_multi_sum_f32')
        return out

    def add_row0(self, dK, dZ):
        """dK [B, n, Cc] (rows with one pitch >= Cc): dK[:, 0, :] += dZ [B, Cc], in place."""
        B, n, Cc = dK.shape
        assert dZ.is_contiguous() and dZ.shape == (B, Cc)
        _chkp3(dK, 'dK')
        self._check(self.lib.qagnn_add_row0_f32(dK.data_ptr(), n * _ld3(dK), dZ.data_ptr(), B, Cc, self._stream()), 'qagnn_add_row0_f32')
        return dK

    def packed_min_rows(self, rows):
        """Tests and A/B runs only: the library's row threshold for packed B images and the three-MFMA form (qagnn_packed_min_rows) and this
        provider's copy of it, together.  Process-wide -- every provider of the process sees it.  Returns the previous value."""
        old = int(self.lib.qagnn_packed_min_rows(int(rows)))
        self.PACK_MIN_M = int(self.lib.qagnn_packed_min_rows(-1))
        return old

    def timing_enable(self, on):
        """Library-side HIP-event brackets around the GEMM and edge-stage entry points (qagnn_timing_enable): measurement harnesses only."""
        self._check(self.lib.qagnn_timing_enable(1 if on else 0), 'qagnn_timing_enable')

    def timing_read(self):
        """-> {kind: (milliseconds, calls)} for 'gemm_nn', 'gemm_tn', 'edge_attn_fwd', 'edge_attn_bwd' since timing_enable(True)"""
        ms, calls = (C.c_double * 4)(), (C.c_int64 * 4)()
        self._check(self.lib.qagnn_timing_read(ms, calls), 'qagnn_timing_read')
        return {k: (ms[i], calls[i]) for i, k in enumerate(('gemm_nn', 'gemm_tn', 'edge_attn_fwd', 'edge_attn_bwd'))}

    def _amax_word_scratch(self, numel, dev):
        """a zeroed int32 [4] maximum word and the scratch of the GELU / dropout passes that leave max |.| of their output in it"""
        word = torch.empty(4, dtype=torch.int32, device=dev)
        self._check(self.lib.qagnn_zero_words(word.data_ptr(), 4, self._stream()), 'qagnn_zero_words')
        return word, torch.empty(self.lib.qagnn_gelu_dropout_amax_scratch_elems(numel), dtype=torch.float32, device=dev)

    def gelu_dropout_fwd(self, X, p, seed, amax=False):
        """amax=True: -> (Y, word) with word = int32 [4], [0] = the bit pattern of max |Y| (qagnn_gelu_dropout_fwd_amax_f32)"""
        assert X.is_contiguous() and X.dtype == torch.float32
        Y = torch.empty_like(X)
        if amax:
            word, scratch = self._amax_word_scratch(X.numel(), X.device)
            self._check(self.lib.qagnn_gelu_dropout_fwd_amax_f32(X.data_ptr(), Y.data_ptr(), X.numel(), float(p), int(seed), word.data_ptr(),
                                                                 scratch.data_ptr(), self._stream()), 'qagnn_gelu_dropout_fwd_amax_f32')
            return Y, word
        self._check(self.lib.qagnn_gelu_dropout_fwd_f32(X.data_ptr(), Y.data_ptr(), X.numel(), float(p), int(seed),
                                                        self._stream()), 'qagnn_gelu_dropout_fwd_f32')
        return Y

    def gelu_dropout_bwd(self, X, dY, p, seed, amax=False):
        """amax=True: -> (dX, word) with word = int32 [4], [0] = the bit pattern of max |dX| (qagnn_gelu_dropout_bwd_amax_f32)"""
        assert X.is_contiguous() and dY.is_contiguous()
        dX = torch.empty_like(X)
        if amax:
            word, scratch = self._amax_word_scratch(X.numel(), X.device)
            self._check(self.lib.qagnn_gelu_dropout_bwd_amax_f32(X.data_ptr(), dY.data_ptr(), dX.data_ptr(), X.numel(), float(p), int(seed),
                                                                 word.data_ptr(), scratch.data_ptr(), self._stream()), 'qagnn_gelu_dropout_bwd_amax_f32')
            return dX, word
        self._check(self.lib.qagnn_gelu_dropout_bwd_f32(X.data_ptr(), dY.data_ptr(), dX.data_ptr(), X.numel(), float(p),
                                                        int(seed), self._stream()), 'qagnn_gelu_dropout_bwd_f32')
        return dX

    def bn_relu_bwd_colsum(self, dR, H, mean, invstd, scale, shift, gamma, red, inv_rows, roww=None, dH=None):
        """bn_relu_bwd that also returns colsum(dH) [Cc]."""
        assert red.is_contiguous() and red.shape == (2, H.size(1))
        dH, ld = self._bn_bwd_operands(dR, H, dH)
        R, Cc = H.shape
        cs = torch.empty(Cc, dtype=torch.float32, device=H.device)
        ws = torch.empty(self.lib.qagnn_colreduce_workspace_elems(R, Cc, 1), dtype=torch.float32, device=H.device)
        rc = self.lib.qagnn_bn_relu_bwd_colsum_f32(dR.data_ptr(), H.data_ptr(), dH.data_ptr(), ld, R, Cc, mean.data_ptr(), invstd.data_ptr(),
                                                   scale.data_ptr(), shift.data_ptr(), gamma.data_ptr(), red[0].data_ptr(), red[1].data_ptr(),
                                                   float(inv_rows), _ptr(roww), cs.data_ptr(), ws.data_ptr(), self._stream())
        self._check(rc, 'qagnn_bn_relu_bwd_colsum_f32')
        return dH, cs

    def sin_basis(self, score, js, ldo):
        assert score.is_contiguous() and js.is_contiguous() and score.dtype == js.dtype == torch.float32
        R, J = score.numel(), js.numel()
        out = torch.empty((R, ldo), dtype=torch.float32, device=score.device)
        self._check(self.lib.qagnn_sin_basis_f32(score.data_ptr(), js.data_ptr(), out.data_ptr(), ldo, R, J, self._stream()),
                    'qagnn_sin_basis_f32')
        return out

    # -- edge kernels -------------------------------------------------------------------------------------------------
    def edge_attn_fwd(self, graph, KMQ, EkEm, HP, qscale, aggr=None):
        """aggr: the [N, DP] output, a view with a pitch of its own (else a contiguous one is allocated)"""
        _chkp(KMQ, 'KMQ'), _chkp(EkEm, 'EkEm')
        DP = 4 * HP
        assert KMQ.shape == (graph.N, 3 * DP) and EkEm.shape == (graph.C, 2 * DP)
        dev = KMQ.device
        a = torch.empty((graph.Ep, 4), dtype=torch.float32, device=dev)
        alpha = torch.empty_like(a)
        if aggr is None:
            aggr = torch.empty((graph.N, DP), dtype=torch.float32, device=dev)
        assert _chkp(aggr, 'aggr').shape == (graph.N, DP)
        score = torch.empty_like(a)  # scratch of the generic kernels (raw scores of hub segments)
        rc = self.lib.qagnn_edge_attn_fwd_f32(C.byref(graph.c), KMQ.data_ptr(), _ld(KMQ), EkEm.data_ptr(), _ld(EkEm), HP, float(qscale), score.data_ptr(),
                                              a.data_ptr(), alpha.data_ptr(), aggr.data_ptr(), _ld(aggr), self._stream())
        self._check(rc, 'qagnn_edge_attn_fwd_f32')
        return aggr, a, alpha

    def edge_attn_bwd(self, graph, KMQ, EkEm, HP, qscale, a, alpha, G, dKMQ=None, dEkEm=None):
        """dKMQ / dEkEm: the outputs; the library writes them with the pitches of KMQ (ldk) and EkEm (lde), so a caller's views must have
        those pitches (else contiguous ones are allocated, which asks KMQ / EkEm to be contiguous)"""
        _chkp(KMQ, 'KMQ'), _chkp(EkEm, 'EkEm'), _chkp(G, 'G')
        DP = 4 * HP
        dev = KMQ.device
        if dKMQ is None:
            dKMQ = torch.empty(KMQ.shape, dtype=torch.float32, device=dev)
        if dEkEm is None:
            dEkEm = torch.empty(EkEm.shape, dtype=torch.float32, device=dev)
        _chkp(dKMQ, 'dKMQ'), _chkp(dEkEm, 'dEkEm')
        assert dKMQ.shape == KMQ.shape and dEkEm.shape == EkEm.shape and G.shape == (graph.N, DP)
        assert _ld(dKMQ) == _ld(KMQ) and _ld(dEkEm) == _ld(EkEm), 'edge_attn_bwd: dKMQ / dEkEm are written with the pitches of KMQ / EkEm'
        ga = torch.empty((graph.Ep, 4), dtype=torch.float32, device=dev)
        rs = torch.empty((graph.N, 4), dtype=torch.float32, device=dev)
        cls_part = torch.empty((graph.cls_part_rows, 2 * DP), dtype=torch.float32, device=dev)
        rc = self.lib.qagnn_edge_attn_bwd_f32(C.byref(graph.c), KMQ.data_ptr(), _ld(KMQ), EkEm.data_ptr(), _ld(EkEm), HP,
                                              float(qscale), a.data_ptr(), alpha.data_ptr(), G.data_ptr(), _ld(G),
                                              dKMQ.data_ptr(), dEkEm.data_ptr(), ga.data_ptr(), rs.data_ptr(),
                                              cls_part.data_ptr(), self._stream())
        self._check(rc, 'qagnn_edge_attn_bwd_f32')
        return dKMQ, dEkEm

    # -- one GATConvE hop per call (csrc/hop.hip) ---------------------------------------------------------------------------
    def _hop_struct(self, graph, HP, qscale, X, S, ntype, prm, batch_stats, eps, p, seed, apply_act, tab_col=-1, side=False, running=None):
        Wx_t, Wx, Ws_t, Ws, TT, EkEm, W1t, W1, b1, gamma, beta, W2t, W2, b2, run_mean_p, run_var_p = prm
        DP = 4 * HP
        _chk2d(X, 'X'), _chk2d(Wx_t, 'Wx_t'), _chk2d(Wx, 'Wx'), _chk2d(TT, 'TT'), _chk2d(EkEm, 'EkEm')
        for t in (W1t, W1, W2t, W2):
            _chk2d(t, 'mlp weight')
        for t in (b1, gamma, beta, b2, run_mean_p, run_var_p):
            assert t.is_contiguous() and t.numel() == DP and t.dtype == torch.float32
        assert X.shape == (graph.N, DP) and Wx_t.shape == (DP, 3 * DP) and Wx.shape == (3 * DP, DP) and EkEm.shape == (graph.C, 2 * DP)
        assert ntype.dtype == torch.long and ntype.numel() == graph.N and ntype.is_contiguous() and TT.size(1) == 3 * DP
        h = qagnn_hop_args()
        h.g = C.pointer(graph.c)
        h.N, h.DP, h.HP, h.T, h.qscale = graph.N, DP, HP, TT.size(0), float(qscale)
        h.X, h.ntype = X.data_ptr(), ntype.data_ptr()
        if S is not None:
            _chk2d(S, 'S'), _chk2d(Ws_t, 'Ws_t'), _chk2d(Ws, 'Ws')
            SP = S.size(1)
            assert S.size(0) == graph.N and Ws_t.shape == (SP, 3 * DP) and Ws.shape == (3 * DP, SP)
            h.SP, h.S, h.Ws_t, h.Ws = SP, S.data_ptr(), Ws_t.data_ptr(), Ws.data_ptr()
        h.Wx_t, h.Wx, h.TT, h.EkEm = Wx_t.data_ptr(), Wx.data_ptr(), TT.data_ptr(), EkEm.data_ptr()
        h.W1t, h.W1, h.b1, h.gamma, h.beta = W1t.data_ptr(), W1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), beta.data_ptr()
        h.W2t, h.W2, h.b2 = W2t.data_ptr(), W2.data_ptr(), b2.data_ptr()
        h.batch_stats, h.eps = (1 if batch_stats else 0), float(eps)
        h.run_mean_p, h.run_var_p = run_mean_p.data_ptr(), run_var_p.data_ptr()
        # (forward only: the train-mode update of the module's running statistics; the hop derives the unbiased-variance factor from N)
        h.run_mean, h.run_var, h.num_batches_tracked, h.dense_pos, h.d, h.momentum, _unb = _running_fields(running)
        h.apply_act, h.p_drop, h.seed = (1 if apply_act else 0), float(p), int(seed)
        h.gemm_split = int(self.gemm_split)
        tc, oc = tab_col if isinstance(tab_col, tuple) else (tab_col, -1)  # (type-indicator column of S, ones column of relu(bn(h1)))
        h.tab_col = int(tc) if S is not None else -1
        h.ones_col = int(oc)
        h.side_stream = self._side_stream() if side else None  # backward only (qagnn_hop_args.side_stream)
        return h

    @staticmethod
    def _set_saved(h, p_kmq, p_aa, p_rows, p_stats, p_amax, Ep, row_b):
        """One hop's saved arrays from the ADDRESSES of its KMQ [N, 3DP], aa [2, Ep, 4] = a | alpha, rows [4, N, DP] = aggr | h1 | out | y,
        stats [5, DP] and maximum words; row_b = the bytes of one [N, DP] matrix.  Addresses by arithmetic: a view tensor per pointer
        costs the host-bound batches ~0.3 ms per step in the stack."""
        h.KMQ, h.stats, h.amax = p_kmq, p_stats, p_amax
        h.a, h.alpha = p_aa, p_aa + Ep * 16
        h.aggr, h.h1, h.out, h.y = (p_rows + i * row_b for i in range(4))

    @staticmethod
    def _grad_sizes(DP, SP, T, n_cls):
        """element counts of dWx_t | dWs_t | dTT | dEkEm | dW1t | db1 | dbn | dW2t | db2 in a hop's flat gradient buffer (each a multiple
        of 4: 16-byte aligned views), and their running offsets"""
        sizes = [DP * 3 * DP, SP * 3 * DP, T * 3 * DP, n_cls * 2 * DP, DP * DP, DP, 2 * DP, DP * DP, DP]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        return sizes, offs

    @staticmethod
    def _carve_grads(h, fl, sizes, offs, n_cls):
        """fl: one hop's flat gradient buffer -> the hop's output pointers, and the ten gradients handed to autograd:
        (dWx_t, dWs_t, dTT, dEkEm, dW1t, db1, dgamma, dbeta, dW2t, db2)."""
        DP, SP, T, base = h.DP, h.SP, h.T, fl.data_ptr()
        h.dWx_t, pdWs_t, h.dTT, h.dEkEm, h.dW1t, h.db1, h.dbn, h.dW2t, h.db2 = (base + o * 4 for o in offs[:9])
        dWx_t, dWs_t, dTT, dEkEm, dW1t, db1, dbn, dW2t, db2 = fl.split(sizes)
        if h.ones_col >= 0:  # the bias gradient IS that row of dW2t, the type-table gradient those rows of dWs_t: views, no copies
            db2 = dW2t.view(DP, DP)[h.ones_col]
            h.db2 = h.dW2t + h.ones_col * DP * 4
        if SP:
            h.dWs_t = pdWs_t
            if h.tab_col >= 0:
                dTT = dWs_t.view(SP, 3 * DP)[h.tab_col:h.tab_col + T]
                h.dTT = pdWs_t + h.tab_col * 3 * DP * 4
        return (dWx_t.view(DP, 3 * DP), dWs_t.view(SP, 3 * DP) if SP else None, dTT.view(T, 3 * DP), dEkEm.view(n_cls, 2 * DP),
                dW1t.view(DP, DP), db1, dbn[DP:], dbn[:DP], dW2t.view(DP, DP), db2)

    def _fwd_ws(self, graph, DP, dev):
        """a hop's forward workspace (the hops of a stack share one): exactly the library's query"""
        return torch.empty(self.lib.qagnn_hop_fwd_workspace_elems(graph.N, graph.Ep, DP), dtype=torch.float32, device=dev)

    def _bwd_ws(self, graph, DP, SP, dev):
        return torch.empty(self.lib.qagnn_hop_bwd_workspace_elems(graph.N, graph.Ep, DP, SP, graph.cls_part_rows), dtype=torch.float32, device=dev)

    def _hop_chain(self, graph, HP, qscale, X, S, ntype, prms, ys, saved, p_amax, x_amax, s_amax, ws, batch_stats, eps, p, seeds, cols, side=False,
                   runnings=None, shared=False):
        """The (qagnn_hop_args * k) of a chained stack: hop l reads X (l = 0) or ys[l - 1] and writes ys[l].  saved = (KMQ, aa, rows, stats) with
        one slot per hop (shared: ONE slot that every hop writes); p_amax: the address of the [k, HOP_AMAX_WORDS] words, or None; x_amax / s_amax:
        the words X's and S's producers left (ops.amax_lookup: no reduction pass then), or None / empty; ws: the workspace the hops share."""
        k, N, DP, Ep = len(prms), graph.N, 4 * HP, graph.Ep
        p_kmq, p_aa, p_rows, p_stats = (t.data_ptr() for t in saved)
        row_b, p_ws, n_ws = N * DP * 4, ws.data_ptr(), ws.numel()
        p_x, p_s = (t.data_ptr() if t is not None and t.numel() else None for t in (x_amax, s_amax))
        hops = (qagnn_hop_args * k)()
        for l in range(k):
            h = self._hop_struct(graph, HP, qscale, X if l == 0 else ys[l - 1], S, ntype, prms[l], batch_stats, eps, p, seeds[l] if seeds else 0, True,
                                 cols, side=side, running=runnings[l] if runnings else None)
            j = 0 if shared else l
            self._set_saved(h, p_kmq + j * 3 * row_b, p_aa + 2 * j * Ep * 16, p_rows + 4 * j * row_b, p_stats + j * 5 * DP * 4,
                            p_amax + l * HOP_AMAX_WORDS * 4 if p_amax else None, Ep, row_b)
            # (one slot per hop: y is where _set_saved put it; the chain hops[l + 1].X == hops[l].y is what shares the amax words)
            h.y, h.x_amax, h.s_amax = ys[l].data_ptr(), (p_x if l == 0 else None), p_s
            h.ws, h.ws_elems = p_ws, n_ws
            hops[l] = h
        return hops

    def hop_fwd(self, graph, HP, qscale, X, S, ntype, prm, batch_stats, eps, p, seed, apply_act, running, cols=-1):
        """-> (y, saved) with saved = (KMQ, aa [2, Ep, 4] = a | alpha, aggr, h1, out, stats [5, DP]); y is `out` when not apply_act."""
        h = self._hop_struct(graph, HP, qscale, X, S, ntype, prm, batch_stats, eps, p, seed, apply_act, cols, running=running)
        N, DP, dev = graph.N, 4 * HP, X.device
        KMQ = torch.empty((N, 3 * DP), dtype=torch.float32, device=dev)
        aa = torch.empty((2, graph.Ep, 4), dtype=torch.float32, device=dev)
        rows = torch.empty((4 if apply_act else 3, N, DP), dtype=torch.float32, device=dev)  # aggr, h1, out (, y)
        stats = torch.empty((5, DP), dtype=torch.float32, device=dev)
        amax = torch.empty(HOP_AMAX_WORDS, dtype=torch.int32, device=dev)  # operand maxima of the three-MFMA form (zeroed by the library)
        ws = self._fwd_ws(graph, DP, dev)
        self._set_saved(h, KMQ.data_ptr(), aa.data_ptr(), rows.data_ptr(), stats.data_ptr(), amax.data_ptr(), graph.Ep, N * DP * 4)
        if not apply_act:
            h.y = None  # (rows has no fourth matrix)
        h.ws, h.ws_elems = ws.data_ptr(), ws.numel()
        self._check(self.lib.qagnn_hop_fwd_f32(C.byref(h), self._stream()), 'qagnn_hop_fwd_f32')
        return rows[3 if apply_act else 2], (KMQ, aa, rows[0], rows[1], rows[2], stats, amax)

    def hop_bwd(self, graph, HP, qscale, X, S, ntype, prm, batch_stats, eps, p, seed, apply_act, saved, dy, need_dX, need_dS,
                dX_acc=None, dS_acc=None, tab_col=-1, overlap=True):
        """-> (dX, dS, dWx_t, dWs_t, dTT, dEkEm, dW1t, db1, dgamma, dbeta, dW2t, db2); overlap: the weight-gradient products on a side stream"""
        h = self._hop_struct(graph, HP, qscale, X, S, ntype, prm, batch_stats, eps, p, seed, apply_act, tab_col, side=overlap)
        KMQ, aa, aggr, h1, out, stats = saved[:6]  # (tensors of their own, e.g. hop_fwd_composed's: no common base to do arithmetic on)
        h.amax = saved[6].data_ptr() if len(saved) > 6 else None
        N, DP, dev, SP = graph.N, 4 * HP, X.device, h.SP
        _chk2d(dy, 'dy')
        h.KMQ, h.a, h.alpha, h.stats = KMQ.data_ptr(), aa[0].data_ptr(), aa[1].data_ptr(), stats.data_ptr()
        h.aggr, h.h1, h.out, h.y = aggr.data_ptr(), h1.data_ptr(), out.data_ptr(), out.data_ptr()
        h.dy = dy.data_ptr()
        sizes, offs = self._grad_sizes(DP, SP, h.T, graph.C)
        grads = self._carve_grads(h, torch.empty(offs[-1], dtype=torch.float32, device=dev), sizes, offs, graph.C)
        dX = dS = None
        if need_dX:  # *_acc: an existing running total of this gradient, added to in place (GEMM epilogue accumulate)
            dX = dX_acc if dX_acc is not None else torch.empty((N, DP), dtype=torch.float32, device=dev)
            assert dX.shape == (N, DP) and dX.is_contiguous()
            h.dX, h.accumulate_dX = dX.data_ptr(), (1 if dX_acc is not None else 0)
        if SP and need_dS:
            dS = dS_acc if dS_acc is not None else torch.empty((N, SP), dtype=torch.float32, device=dev)
            assert dS.shape == (N, SP) and dS.is_contiguous()
            h.dS, h.accumulate_dS = dS.data_ptr(), (1 if dS_acc is not None else 0)
        ws = self._bwd_ws(graph, DP, SP, dev)
        h.ws, h.ws_elems = ws.data_ptr(), ws.numel()
        self._check(self.lib.qagnn_hop_bwd_f32(C.byref(h), self._stream()), 'qagnn_hop_bwd_f32')
        return (dX, dS, *grads)

    # -- the forward-only path (include/qagnn_hip_infer.h) ----------------------------------------------------------------------------------
    def bn_relu_absmax(self, H, scale, shift, out=None):
        """max relu(scale * H + shift) merged into out[0] (int32 [>= 1]; None: a zeroed int32 [4] is allocated); H [R, Cc], rows may be pitched"""
        _chkp(H, 'H')
        R, Cc = H.shape
        assert scale.is_contiguous() and shift.is_contiguous() and scale.numel() == shift.numel() == Cc and scale.dtype == shift.dtype == torch.float32
        if out is None:
            out = torch.empty(4, dtype=torch.int32, device=H.device)
            self._check(self.lib.qagnn_zero_words(out.data_ptr(), 4, self._stream()), 'qagnn_zero_words')
        assert out.dtype == torch.int32 and out.is_cuda
        scratch = torch.empty(max(int(self.lib.qagnn_bn_relu_absmax_scratch_elems(R, Cc)), 1), dtype=torch.float32, device=H.device)
        self._check(self.lib.qagnn_bn_relu_absmax_f32(H.data_ptr(), _ld(H), R, Cc, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                                      self._stream()), 'qagnn_bn_relu_absmax_f32')
        return out

    def choice_eval(self, logits, labels, counts, pred=None):
        """logits [Q, nc] fp32 (rows may be pitched), labels int64 [Q] or None, counts int64 [2] = (correct, seen), added to in place;
        pred: int64 [Q] to receive the argmax, or None.  No synchronisation (qagnn_choice_eval_f32)."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        Q, nc = logits.shape
        assert counts.dtype == torch.long and counts.numel() == 2 and counts.is_contiguous() and counts.is_cuda
        assert labels is None or (labels.dtype == torch.long and labels.numel() == Q and labels.is_contiguous() and labels.is_cuda)
        assert pred is None or (pred.dtype == torch.long and pred.numel() == Q and pred.is_contiguous() and pred.is_cuda)
        self._check(self.lib.qagnn_choice_eval_f32(logits.data_ptr(), _ld(logits), _ptr(labels), Q, nc, _ptr(pred), counts.data_ptr(), self._stream()),
                    'qagnn_choice_eval_f32')
        return counts

    # -- the training losses (include/qagnn_hip_loss.h) ---------------------------------------------------------------------------------------
    def zero_words(self, t):
        """zero a contiguous device tensor of 4-byte-multiple size with the library's own kernel (qagnn_zero_words): no memset node in a capture"""
        nbytes = t.numel() * t.element_size()
        assert t.is_cuda and t.is_contiguous() and nbytes % 4 == 0
        self._check(self.lib.qagnn_zero_words(t.data_ptr(), nbytes // 4, self._stream()), 'qagnn_zero_words')
        return t

    def _loss_flag_word(self, device):
        # ONE persistent flag word per device (no zeroing launch per call): ERR_WATCH clears it once it has reported it (`reset`)
        flags = self._loss_flags.get(device)
        if flags is None:
            flags = self._loss_flags[device] = torch.zeros(4, dtype=torch.int32, device=device)
        return flags

    def choice_loss(self, logits, labels, kind='cross_entropy', margin=0.1, weight=None, stats=None, g=None):
        """-> (loss fp32 [1], g [Q, nc] = d loss / d logits) in one launch (qagnn_choice_loss_f32).  logits [Q, nc] fp32, rows may be pitched;
        labels int64 [Q]; weight: a one-element fp32 device tensor or None (= 1); stats: float64 [2] = (sum of losses, calls), added to in
        place, or None; g: a [Q, nc] fp32 view to receive the gradient (rows may be pitched), else allocated.  A label outside [0, nc) is
        reported through ERR_WATCH: it raises one call late, or at poll(block=True).  No synchronisation."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and (logits.stride(1) == 1 or logits.size(1) == 1)
        Q, nc = logits.shape
        dev = logits.device
        assert labels.dtype == torch.long and labels.numel() == Q and labels.is_contiguous() and labels.device == dev
        if weight is not None:
            self._check_scale_word(weight, dev)
        assert stats is None or (stats.dtype == torch.float64 and stats.numel() == 2 and stats.is_contiguous() and stats.device == dev)
        if g is None:
            g = torch.empty((Q, nc), dtype=torch.float32, device=dev)
        assert g.dtype == torch.float32 and g.shape == (Q, nc) and g.device == dev and (g.stride(1) == 1 or nc == 1)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        flags = self._loss_flag_word(dev)
        rc = self.lib.qagnn_choice_loss_f32(logits.data_ptr(), _ld(logits), labels.data_ptr(), Q, nc, LOSS_KINDS[kind], float(margin), _ptr(weight),
                                            loss.data_ptr(), g.data_ptr(), _ld(g), _ptr(stats), flags.data_ptr(), self._stream())
        self._check(rc, 'qagnn_choice_loss_f32')
        ERR_WATCH.poll()
        ERR_WATCH.watch(flags, f'labels (a label outside the {nc} choices)', reset=flags)
        return loss, g

    def choice_loss_bwd(self, g, grad_out, out=None):
        """-> dlogits = g * grad_out[0] (qagnn_choice_loss_bwd_f32); grad_out: a one-element fp32 device tensor; out: g itself or a [Q, nc] view"""
        assert g.is_cuda and g.dtype == torch.float32 and g.dim() == 2 and (g.stride(1) == 1 or g.size(1) == 1)
        self._check_scale_word(grad_out, g.device)
        Q, nc = g.shape
        if out is None:
            out = torch.empty((Q, nc), dtype=torch.float32, device=g.device)
        assert out.dtype == torch.float32 and out.shape == (Q, nc) and out.device == g.device and (out.stride(1) == 1 or nc == 1)
        self._check(self.lib.qagnn_choice_loss_bwd_f32(g.data_ptr(), _ld(g), grad_out.data_ptr(), out.data_ptr(), _ld(out), Q, nc, self._stream()),
                    'qagnn_choice_loss_bwd_f32')
        return out

    # -- the trainable entity table's gradient (include/qagnn_hip_rows.h).  The caller owns every output and workspace: nothing is allocated here
    def row_groups_workspace_elems(self, N):
        """int32 words of workspace row_groups() needs for N positions"""
        return int(self.lib.qagnn_row_groups_workspace_elems(int(N)))

    def row_groups(self, ridx, table_rows, order, seg, uniq, count, workspace):
        """ridx int64 [N] -> order int32 [N], seg int32 [N + 1], uniq int64 [N], count int32 [1]: the positions with 0 <= ridx < table_rows
        grouped by row id (qagnn_row_groups).  workspace: int32, at least row_groups_workspace_elems(N) words.  No synchronisation."""
        N = ridx.numel()
        dev = ridx.device
        assert ridx.is_cuda and ridx.dtype == torch.long and ridx.is_contiguous()
        for t, dt, ne in ((order, torch.int32, N), (seg, torch.int32, N + 1), (uniq, torch.long, N), (count, torch.int32, 1), (workspace, torch.int32, 0)):
            assert t.device == dev and t.dtype == dt and t.is_contiguous() and t.numel() >= ne
        self._check(self.lib.qagnn_row_groups(ridx.data_ptr(), N, int(table_rows), order.data_ptr(), seg.data_ptr(), uniq.data_ptr(), count.data_ptr(),
                                              workspace.data_ptr(), workspace.numel(), self._stream()), 'qagnn_row_groups')
        return order, seg, uniq, count

    def row_segment_sum_workspace_elems(self, N, cols):
        """floats of workspace row_segment_sum() needs for N positions of `cols` floats"""
        return int(self.lib.qagnn_row_segment_sum_workspace_elems(int(N), int(cols)))

    def row_segment_sum(self, X, order, seg, count, G, workspace):
        """G[u] = the sum of X[order[j]] over group u in the fixed order of include/qagnn_hip_rows.h, zeros from row *count on
        (qagnn_row_segment_sum_f32).  X [N, cols], G [g_rows <= N, cols]: fp32, rows may be pitched; workspace: fp32."""
        _chkp(X, 'X'), _chkp(G, 'G')
        N, cols = X.shape
        assert G.size(1) == cols and order.dtype == torch.int32 and seg.dtype == torch.int32 and count.dtype == torch.int32
        assert order.numel() >= N and seg.numel() >= N + 1 and order.is_contiguous() and seg.is_contiguous() and workspace.dtype == torch.float32
        self._check(self.lib.qagnn_row_segment_sum_f32(X.data_ptr(), _ld(X), cols, order.data_ptr(), seg.data_ptr(), count.data_ptr(), N, G.data_ptr(),
                                                       _ld(G), G.size(0), workspace.data_ptr(), workspace.numel(), self._stream()),
                    'qagnn_row_segment_sum_f32')
        return G

    def rows_scatter(self, R, uniq, count, out, accumulate=False):
        """out[uniq[u]] = R[u] (or +=) for u < min(*count, rows of R); no other word of `out` is touched (qagnn_rows_scatter_f32).
        R [n_rows, cols], out [table_rows, cols]: fp32, rows may be pitched; uniq int64 [>= n_rows], ids distinct."""
        _chkp(R, 'R'), _chkp(out, 'out')
        assert R.size(1) == out.size(1) and uniq.dtype == torch.long and uniq.is_contiguous() and uniq.numel() >= R.size(0) and count.dtype == torch.int32
        self._check(self.lib.qagnn_rows_scatter_f32(R.data_ptr(), _ld(R), R.size(1), uniq.data_ptr(), count.data_ptr(), R.size(0), out.data_ptr(), _ld(out),
                                                    out.size(0), 1 if accumulate else 0, self._stream()), 'qagnn_rows_scatter_f32')
        return out

    def stack_infer(self, graph, HP, qscale, X, S, ntype, prms, eps, cols=-1, x_amax=None, s_amax=None, keep=False, attn=False):
        """The k-hop forward with running statistics and no dropout that keeps nothing (qagnn_stack_infer_f32): ONE set of hop buffers shared
        by all hops plus two alternating y.  -> (y [N, DP], amax [k, HOP_AMAX_WORDS]).  keep=True (tests): a set of buffers per hop, returned
        as a third value (KMQ, aa, rows, stats) laid out as stack_fwd's saved tensors.  attn=True (ops.attention_capture): one `a` buffer PER
        HOP, returned as a third value [k, Ep, 4] in source order; everything else stays shared -- the same launches, only the address of a
        differs."""
        assert not (keep and attn)
        k = len(prms)
        N, DP, Ep, dev = graph.N, 4 * HP, graph.Ep, X.device
        kk = k if keep else 1
        KMQ = torch.empty((kk, N, 3 * DP), dtype=torch.float32, device=dev)
        aa = torch.empty((kk, 2, Ep, 4), dtype=torch.float32, device=dev)
        rows = torch.empty((kk, 4, N, DP), dtype=torch.float32, device=dev) if keep else torch.empty((5, N, DP), dtype=torch.float32, device=dev)
        stats = torch.empty((kk, 5, DP), dtype=torch.float32, device=dev)
        amax = torch.empty((k, HOP_AMAX_WORDS), dtype=torch.int32, device=dev)
        ws = self._fwd_ws(graph, DP, dev)
        ys = [rows[l, 3] if keep else rows[3 + (l & 1)] for l in range(k)]  # (shared set: aggr | h1 | out | y even | y odd)
        hops = self._hop_chain(graph, HP, qscale, X, S, ntype, prms, ys, (KMQ, aa, rows, stats), amax.data_ptr(), x_amax, s_amax, ws, False, eps, 0.0,
                               None, cols, shared=not keep)
        if attn:
            a_all = torch.empty((k, Ep, 4), dtype=torch.float32, device=dev)
            for l in range(k):
                hops[l].a = a_all.data_ptr() + l * Ep * 16
        self._check(self.lib.qagnn_stack_infer_f32(hops, k, self._stream()), 'qagnn_stack_infer_f32')
        if attn:
            return ys[-1], amax, a_all
        return (ys[-1], amax, (KMQ, aa, rows, stats)) if keep else (ys[-1], amax)

    # -- the detailed evaluation (include/qagnn_hip_explain.h) ------------------------------------------------------------------------------
    @staticmethod
    def _chk_attn(graph, a):
        """a: [k, Ep, 4] fp32 in source order, layers a multiple of 4 floats (>= 4 Ep) apart, rows contiguous -> (k, layer stride)"""
        assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 3 and a.shape[1:] == (graph.Ep, 4), \
            f'a: need a [k, Ep = {graph.Ep}, 4] float32 device tensor, got {tuple(a.shape)} {a.dtype} {a.device}'
        k = a.size(0)
        ls = a.stride(0) if k > 1 else 4 * graph.Ep
        assert k == 0 or ((graph.Ep == 1 or a.stride(1) == 4) and a.stride(2) == 1 and ls >= 4 * graph.Ep and ls % 4 == 0 and a.data_ptr() % 16 == 0), \
            f'a: rows of 4 contiguous floats, layers a multiple of 4 floats apart, 16-byte aligned; got strides {a.stride()}'
        return k, ls

    def attn_export(self, graph, a, out=None):
        """a [k, Ep, 4] (the hops' pre-degree softmax in source order; layers may be pitched) -> alpha [k, Ep, 4] in the caller's edge order, self
        loops last: alpha[l][eid_s[p]] = a[l][p] for the rowptr_s[N] live positions, one launch (qagnn_attn_export_f32).  Rows behind the
        live ones (a graph with an edge capacity) are not written.  out: a [k, Ep, 4] tensor to write into (layers may be pitched), else
        allocated."""
        k, ls = self._chk_attn(graph, a)
        if out is None:
            out = torch.empty((k, graph.Ep, 4), dtype=torch.float32, device=a.device)
        ko, ols = self._chk_attn(graph, out)
        assert ko == k and out.device == a.device
        self._check(self.lib.qagnn_attn_export_f32(C.byref(graph.c), a.data_ptr() if k else None, ls, k, out.data_ptr() if k else None, ols,
                                                   self._stream()), 'qagnn_attn_export_f32')
        return out

    def attn_trace(self, graph, a, B, n, root=0, head=-1, out=None):
        """-> (flow [k + 1, N], best [k + 1, N], pred [k, N] int32): the attention a [k, Ep, 4] followed out of node slot `root` of each of
        the B subgraphs of n node rows, one launch (qagnn_attn_trace_f32).  head: -1 the mean of the four heads, or one head.  out: the
        three tensors to write into, else allocated."""
        k, ls = self._chk_attn(graph, a)
        N, dev = graph.N, a.device
        if out is None:
            out = (torch.empty((k + 1, N), dtype=torch.float32, device=dev), torch.empty((k + 1, N), dtype=torch.float32, device=dev),
                   torch.empty((k, N), dtype=torch.int32, device=dev))
        flow, best, pred = out
        for t, rows, dt in ((flow, k + 1, torch.float32), (best, k + 1, torch.float32), (pred, k, torch.int32)):
            assert t.is_cuda and t.dtype == dt and t.shape == (rows, N) and t.is_contiguous() and t.device == dev
        self._check(self.lib.qagnn_attn_trace_f32(C.byref(graph.c), a.data_ptr() if k else None, ls, k, int(B), int(n), int(root), int(head),
                                                  flow.data_ptr(), best.data_ptr(), pred.data_ptr() if k else None, self._stream()),
                    'qagnn_attn_trace_f32')
        return flow, best, pred

    # -- the whole k-hop stack per call (csrc/hop.hip: qagnn_stack_{fwd,bwd}_f32) -------------------------------------------------------
    def stack_fwd(self, graph, HP, qscale, X, S, ntype, prms, batch_stats, eps, p, seeds, runnings, cols=-1, x_amax=None, s_amax=None):
        """k hops with GELU + dropout after each; prms / seeds / runnings: per-layer lists.  -> (y [N, DP], saved)."""
        k = len(prms)
        N, DP, Ep, dev = graph.N, 4 * HP, graph.Ep, X.device
        KMQ = torch.empty((k, N, 3 * DP), dtype=torch.float32, device=dev)
        aa = torch.empty((k, 2, Ep, 4), dtype=torch.float32, device=dev)
        rows = torch.empty((k, 4, N, DP), dtype=torch.float32, device=dev)  # per hop: aggr, h1, out, y
        stats = torch.empty((k, 5, DP), dtype=torch.float32, device=dev)
        amax = torch.empty((k, HOP_AMAX_WORDS), dtype=torch.int32, device=dev)  # one array: the library zeroes it with one launch
        ws = self._fwd_ws(graph, DP, dev)
        ys = rows[:, 3].unbind(0)
        hops = self._hop_chain(graph, HP, qscale, X, S, ntype, prms, ys, (KMQ, aa, rows, stats), amax.data_ptr(), x_amax, s_amax, ws, batch_stats, eps, p,
                               seeds, cols, runnings=runnings)
        self._check(self.lib.qagnn_stack_fwd_f32(hops, k, self._stream()), 'qagnn_stack_fwd_f32')
        ext = torch.empty(0, dtype=torch.int32, device=dev)
        return ys[k - 1], (KMQ, aa, rows, stats, amax, x_amax if x_amax is not None else ext, s_amax if s_amax is not None else ext)

    def stack_bwd(self, graph, HP, qscale, X, S, ntype, prms, batch_stats, eps, p, seeds, saved, dy, need_dX, need_dS, dX_acc=None, tab_col=-1,
                  overlap=True, defer=True):
        """-> (dX, dS, [per layer: (dWx_t, dWs_t, dTT, dEkEm, dW1t, db1, dgamma, dbeta, dW2t, db2)]); dX_acc: an existing running total of
        the stack input's gradient (the output GEMM's share), added to in place.  defer: dEkEm and db1 of all layers are reduced once,
        behind the last hop (qagnn_stack_bwd_deferred_f32: bit-identical to qagnn_stack_bwd_f32, which defer=False calls)."""
        k = len(prms)
        KMQ, aa, rows, stats = saved[:4]
        p_amax = saved[4].data_ptr() if len(saved) > 4 else None
        x_amax, s_amax = (saved[5], saved[6]) if len(saved) > 6 else (None, None)
        N, DP, Ep, dev = graph.N, 4 * HP, graph.Ep, X.device
        SP = S.size(1) if S is not None else 0
        _chk2d(dy, 'dy')
        sizes, offs = self._grad_sizes(DP, SP, prms[0][4].size(0), graph.C)
        per = offs[-1]
        flat = torch.empty(k * per, dtype=torch.float32, device=dev)
        dxs = torch.empty((max(k - 1, 1), N, DP), dtype=torch.float32, device=dev)  # gradient handed from hop l to hop l-1
        dS = torch.empty((N, SP), dtype=torch.float32, device=dev) if (SP and need_dS) else None
        dX = None
        if need_dX:
            dX = dX_acc if dX_acc is not None else torch.empty((N, DP), dtype=torch.float32, device=dev)
            assert dX.shape == (N, DP) and dX.is_contiguous()
        ws = self._bwd_ws(graph, DP, SP, dev)
        hops = self._hop_chain(graph, HP, qscale, X, S, ntype, prms, rows[:, 3].unbind(0), (KMQ, aa, rows, stats), p_amax, x_amax, s_amax, ws,
                               batch_stats, eps, p, seeds, tab_col, side=overlap)
        grads, p_dxs, row_b = [], dxs.data_ptr(), N * DP * 4
        for l, h in enumerate(hops):
            h.dy = dy.data_ptr() if l == k - 1 else p_dxs + l * row_b
            grads.append(self._carve_grads(h, flat[l * per:(l + 1) * per], sizes, offs, graph.C))
            if l > 0:
                h.dX, h.accumulate_dX = p_dxs + (l - 1) * row_b, 0
            elif dX is not None:
                h.dX, h.accumulate_dX = dX.data_ptr(), (1 if dX_acc is not None else 0)
            if dS is not None:
                h.dS, h.accumulate_dS = dS.data_ptr(), (0 if l == k - 1 else 1)  # hop k-1's backward runs first
        if defer and k <= DEFER_MAX_HOPS:  # (the hops of this chain share one graph and one shape: what the deferral asks for)
            dws = torch.empty(self.lib.qagnn_stack_bwd_defer_elems(N, DP, graph.cls_part_rows, k), dtype=torch.float32, device=dev)
            self._check(self.lib.qagnn_stack_bwd_deferred_f32(hops, k, dws.data_ptr(), dws.numel(), self._stream()), 'qagnn_stack_bwd_deferred_f32')
        else:
            self._check(self.lib.qagnn_stack_bwd_f32(hops, k, self._stream()), 'qagnn_stack_bwd_f32')
        return dX, dS, grads
