"""ctypes binding of include/ext/qagnn_hip_step.h: the tail of a captured training step (window accumulation, the RAdam update with its
hyper-parameters in device records).

The header waits in include/ext/ until the pinned inventory of include/*.h is next revised (the header says so itself), so its entry
points are declared here, on a second ctypes handle of the same libqagnn_hip.so, and are no methods of _lib.HipKernels.  Every method
takes every buffer from its caller: nothing is allocated here, so nothing here can hand out an undefined word.
"""
import ctypes as C
import os

import torch

from . import _abi, _lib

HEADER = _abi.header(os.path.join(_abi.INCLUDE, 'ext', 'qagnn_hip_step.h'))
EXPORTS_STEP = HEADER.names
STEP_VERSION = HEADER.define('QAGNN_STEP_VERSION')
RECORD_WORDS = HEADER.define('QAGNN_STEP_RECORD_WORDS')
qagnn_step_record = HEADER.structs['qagnn_step_record']
assert C.sizeof(qagnn_step_record) == 4 * RECORD_WORDS
RECORD_FIELDS = ('decay', 's', 'mode', 'beta1', 'beta2', 'ob1', 'ob2', 'eps')


def load_step_library(path=None):
    """a handle of its own on libqagnn_hip.so with the prototypes of qagnn_hip_step.h declared (and qagnn_grad_norm_f32 of qagnn_hip.h, which
    the captured tail calls on caller-owned buffers).  OSError if the library has not been built or lacks one of them."""
    path = path or _lib.LIB_PATH
    if not os.path.exists(path):
        raise OSError(f'{path} not found: build it with `python -m qagnn_amd.build` (hipcc, gfx950)')
    lib = C.CDLL(path)
    norm = [p for p in _lib._MAIN.prototypes if p[0] in ('qagnn_grad_norm_f32', 'qagnn_grad_norm_workspace_elems', 'qagnn_last_error')]
    for name, restype, argtypes in HEADER.prototypes + norm:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise OSError(f'{path} does not export {name}, which include/ext/qagnn_hip_step.h declares: rebuild it with '
                          '`python -m qagnn_amd.build --force`') from None
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def pack_records(values):
    """[{decay, s, mode, beta1, beta2, ob1, ob2, eps}, ...] (optimization_utils.radam_record) -> a host array of qagnn_step_record.  The
    doubles are rounded to fp32 here, once, by the C conversion -- what `(float)` does to the arguments of qagnn_radam_step_scaled_f32."""
    arr = (qagnn_step_record * max(len(values), 1))()
    for r, val in zip(arr, values):
        for k in RECORD_FIELDS:
            setattr(r, k, val[k])
    return arr


def _table(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _numel(ts):
    return (C.c_int64 * len(ts))(*[t.numel() for t in ts])


def _check_list(ts, n, dev, what):
    assert len(ts) == n and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in ts), \
        f'{what}: need {n} contiguous fp32 tensors on {dev}'


class StepKernels:
    """Tensor-level calls into the entry points of qagnn_hip_step.h, each on the current HIP stream of its operands' device."""

    def __init__(self, path=None):
        if not torch.cuda.is_available():
            raise RuntimeError('qagnn_amd needs an MI355X: torch.cuda.is_available() is False and there is no CPU fallback')
        self.lib = load_step_library(path)
        if self.lib.qagnn_step_version() != STEP_VERSION:
            raise RuntimeError('libqagnn_hip.so: qagnn_hip_step.h version mismatch')

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f'{what} failed (code {rc}): {self.lib.qagnn_last_error().decode()}')

    @staticmethod
    def _stream(dev):
        return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())

    @staticmethod
    def _records_ptr(records, n_records):
        assert records.is_cuda and records.dtype == torch.float32 and records.is_contiguous() and records.numel() >= n_records * RECORD_WORDS \
            and records.data_ptr() % 16 == 0, f'records: a contiguous fp32 device tensor of at least {n_records} x {RECORD_WORDS} words'
        return C.cast(records.data_ptr(), C.POINTER(qagnn_step_record))

    def records_write(self, records, values, first=0):
        """records[first + i] = values[i]: `records` a caller-owned fp32 device tensor of RECORD_WORDS words per record (torch.zeros: a record
        starts defined), `values` what pack_records() takes or returns.  The values travel in the launches' arguments."""
        arr = values if isinstance(values, C.Array) else pack_records(values)
        n = len(values)
        with torch.cuda.device(records.device):
            self._check(self.lib.qagnn_step_records_write(self._records_ptr(records, first + n), int(first), n, arr, self._stream(records.device)),
                        'qagnn_step_records_write')

    def radam_step_records(self, params, grads, exp_avgs, exp_avg_sqs, rec_index, records, grad_scale=None):
        """The fused RAdam update of _lib.HipKernels.radam_step with tensor i's scalars read from record rec_index[i] of `records` when the
        kernels run (qagnn_radam_step_records_f32).  grad_scale: a one-element fp32 device tensor, or None."""
        n = len(params)
        if n == 0:
            return
        dev = params[0].device
        for group, what in ((params, 'params'), (grads, 'grads'), (exp_avgs, 'exp_avgs'), (exp_avg_sqs, 'exp_avg_sqs')):
            _check_list(group, n, dev, what)
        assert all(p.numel() == g.numel() == m.numel() == v.numel() for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs))
        assert len(rec_index) == n
        n_records = records.numel() // RECORD_WORDS
        scale = None
        if grad_scale is not None:
            _lib.HipKernels._check_scale_word(grad_scale, dev)
            scale = grad_scale.data_ptr()
        with torch.cuda.device(dev):
            rc = self.lib.qagnn_radam_step_records_f32(n, _table(params), _table(grads), _table(exp_avgs), _table(exp_avg_sqs), _numel(params),
                                                       (C.c_int32 * n)(*[int(i) for i in rec_index]), self._records_ptr(records, n_records),
                                                       n_records, scale, self._stream(dev))
        self._check(rc, 'qagnn_radam_step_records_f32')

    def window_accumulate(self, dst, src, first):
        """dst[i] = src[i] where the device word `first` (int32 [1]) is non-zero, else dst[i] + src[i] (qagnn_window_accumulate_f32)"""
        n = len(dst)
        if n == 0:
            return
        dev = dst[0].device
        _check_list(dst, n, dev, 'dst'), _check_list(src, n, dev, 'src')
        assert all(d.numel() == s.numel() for d, s in zip(dst, src))
        assert first.is_cuda and first.dtype == torch.int32 and first.numel() == 1 and first.device == dev, 'first: a one-element int32 device tensor'
        with torch.cuda.device(dev):
            rc = self.lib.qagnn_window_accumulate_f32(n, _table(dst), _table(src), _numel(dst), first.data_ptr(), self._stream(dev))
        self._check(rc, 'qagnn_window_accumulate_f32')

    def grad_norm_workspace_elems(self, grads):
        return int(self.lib.qagnn_grad_norm_workspace_elems(len(grads), _numel(grads)))

    def grad_norm_into(self, grads, max_norm, workspace, out2):
        """_lib.HipKernels.grad_norm into caller-owned static buffers: out2 fp32 [2] = (norm, clip coefficient), workspace of at least
        grad_norm_workspace_elems(grads) fp32 elements (qagnn_grad_norm_f32 of qagnn_hip.h: capturable as it is)"""
        n = len(grads)
        dev = out2.device
        _check_list(grads, n, dev, 'grads')
        need = self.grad_norm_workspace_elems(grads)
        assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.device == dev \
            and workspace.numel() >= need, f'grad_norm_into: need {need} fp32 workspace elements on {dev}'
        assert out2.dtype == torch.float32 and out2.is_contiguous() and out2.numel() >= 2
        with torch.cuda.device(dev):
            rc = self.lib.qagnn_grad_norm_f32(n, _table(grads), _numel(grads), float(max_norm), workspace.data_ptr(), out2.data_ptr(), self._stream(dev))
        self._check(rc, 'qagnn_grad_norm_f32')


_KERNELS = None


def kernels():
    """the process's StepKernels (built on first use)"""
    global _KERNELS
    if _KERNELS is None:
        _KERNELS = StepKernels()
    return _KERNELS
