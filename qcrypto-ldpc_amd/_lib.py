"""The one load of ``libqldpc.so`` and what every module of the binding does with a call: signatures, pointer types, the error, handles,
streams and device tensors as arguments."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QLDPC_LIB") or os.path.join(_HERE, "libqldpc.so")      # QLDPC_LIB: A/B builds of the same library

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libqldpc.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
        "`make -C qcrypto-ldpc_amd/csrc`. There is no CPU fallback." % LIB_PATH)

def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (soname libamdhip64.so.7, requested by file name).
    If libqldpc pulled /opt/rocm's copy in first, a later `import torch` would load a SECOND HIP runtime and
    whichever initialises last sees no GPU.  Loading torch's copy first makes both share one runtime."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


_preload_torch_hip_runtime()
_L = C.CDLL(LIB_PATH)

_ip = C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p


def _sig(name, res, args):
    f = getattr(_L, name)
    f.restype = res
    f.argtypes = args
    return f


_sig("qldpc_strerror", C.c_char_p, [C.c_int])
_sig("qldpc_last_error", C.c_char_p, [])


class QldpcError(RuntimeError):
    """Raised where the AFF3CT objects would throw tools::exception; carries the C status."""

    def __init__(self, status, where):
        self.status = status
        msg = _L.qldpc_last_error().decode(errors="replace")
        super().__init__("%s: %s (%d)%s" % (where, _L.qldpc_strerror(status).decode(), status, (": " + msg) if msg else ""))


def _chk(rc, where):
    if rc < 0:
        raise QldpcError(rc, where)
    return rc


def _np_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


def _torch():
    import torch
    return torch


# ---- what the classes of the binding share: a handle's lifetime, a cfg's defaults, streams and device tensors as arguments ------------------

class _Handle:
    """An object of the library: its handle `_h` and the call that frees it (`_free`, set by the class)."""

    def __del__(self):
        try:
            self._free(self._h)
        except Exception:      # a constructor that raised, or the interpreter shutting down
            pass


def _default(cfg_type, default_fn):
    """a cfg structure with the library's defaults"""
    cfg = cfg_type()
    default_fn(C.byref(cfg))
    return cfg


def _create(who, create_fn, *args):
    """the handle a create call writes through its last argument"""
    h = _vp()
    _chk(create_fn(*args, C.byref(h)), who)
    return h


def _stream_arg(stream, device):
    """`stream`, or torch's current stream on `device`, as the argument of a call"""
    s = stream if stream is not None else _torch().cuda.current_stream(device)
    return _vp(s.cuda_stream)


def _dev_rows(t, rows, cols, dtypes, name):
    """a device tensor [rows, cols] (rows None: any number) of one of `dtypes`, a packed-row tensor as a rule -> its pointer; None stays None"""
    if t is None:
        return None
    assert t.is_cuda and t.dtype in dtypes and t.is_contiguous() and t.dim() == 2 and t.shape[1] == cols and rows in (None, t.shape[0]), name
    return _vp(t.data_ptr())


def _dev_vec(t, n, dtype, name):
    """a per-frame or per-VN device vector of n entries -> its pointer; None stays None"""
    if t is None:
        return None
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == n, name
    return _vp(t.data_ptr())


def _dev_empty(device, shape, dtype):
    """a fresh output tensor on `device` (an index or a torch.device)"""
    return _torch().empty(shape, dtype=dtype, device="cuda:%d" % device if isinstance(device, int) else device)
