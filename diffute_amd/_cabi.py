"""ctypes binding of the gfx950 C-ABI library (include/diffute_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  Nothing under oracle/ is ever imported from here.
"""
import ctypes
import os
from ctypes import c_void_p

from . import _cheader

# DIFFUTE_HIP_LIB: A/B builds of the same library (kernel experiments); the default is the in-tree build
_LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
_LIB_PATH = os.environ.get("DIFFUTE_HIP_LIB") or os.path.join(_LIB_DIR, "libdiffute_hip.so")
# the same sources compiled with -DDMX_F16: fp16 storage / MFMA operands (BASELINE configs[4]; `.to(dtype=torch.float16)`)
_LIB_PATH_F16 = os.environ.get("DIFFUTE_HIP_LIB_F16") or os.path.join(_LIB_DIR, "libdiffute_hip_f16.so")
_lib = None
_lib_f16 = None
_exclusive = None        # set_exclusive_device(): None = the library default (1)
_last_elem = "bf16"      # the build handed out last: check() reads ITS error message (the call that failed went through it)


# The binding is derived from the public header at import (_cheader.py): the structures (GemmDesc, UNetConfig, EditItem, ...: CamelCase of
# the header name without `dmx_`), _PROTOS = {symbol: (restype, [argtypes])} and the integer constants (DMX_SCHED_DDIM -> SCHED_DDIM).
# Adding an entry to the ABI takes its declaration in the header and its definition in csrc/, nothing here.
_HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffute_hip.h")
_CLASS_NAMES = {"dmx_unet_config": "UNetConfig", "dmx_vae_config": "VAEConfig", "dmx_vit_config": "ViTConfig", "dmx_trocr_dec_config": "TrOCRDecConfig"}


def _read_header():
    if not os.path.exists(_HEADER_PATH):
        raise RuntimeError(f"diffute_amd: the C-ABI header is missing ({_HEADER_PATH}). The binding is derived from it at import; "
                           "use the package from its source tree. There is no CPU fallback.")
    with open(_HEADER_PATH) as f:
        return _cheader.parse(f.read(), _CLASS_NAMES)


_abi = _read_header()
_PROTOS = _abi.protos
globals().update({cls.__name__: cls for cls in _abi.structs.values()})
globals().update({n[4:]: _abi.constant(n) for n in list(_abi.macros) + list(_abi.enums) if n.startswith("DMX_")})
# short names of the decoder's beam state block and state words (DMX_TROCR_BEAM_*, DMX_TROCR_STATE_*)
globals().update({n[6:]: v for n, v in list(globals().items()) if n.startswith(("TROCR_BEAM_", "TROCR_STATE_"))})


def lib_path():
    return _LIB_PATH


def _load(path, want_elem):
    if not os.path.exists(path):
        raise RuntimeError(
            f"diffute_amd: HIP extension not built ({path} missing). "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C diffute_amd/csrc`. "
            "There is no CPU fallback.")
    l = ctypes.CDLL(path)                  # RTLD_LOCAL: the two builds export the same names and must not see each other
    for name, (res, args) in _PROTOS.items():
        fn = getattr(l, name)              # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    got = l.dmx_element_type().decode()
    if got != want_elem:
        raise RuntimeError(f"diffute_amd: {path} computes in {got}, expected the {want_elem} build")
    if _exclusive is not None:
        l.dmx_set_exclusive_device(1 if _exclusive else 0)
    return l


def lib(elem="bf16"):
    """Load (once) and return the C-ABI library - the bf16 build, or with elem="fp16" the fp16 build of the same sources;
    raises if it has not been built."""
    global _lib, _lib_f16, _last_elem
    if elem == "fp16":
        if _lib_f16 is None:
            _lib_f16 = _load(_LIB_PATH_F16, "fp16")
        _last_elem = "fp16"
        return _lib_f16
    if elem != "bf16":
        raise ValueError(f"diffute_amd: no build for element type {elem!r}")
    if _lib is None:
        _lib = _load(_LIB_PATH, "bf16")
    _last_elem = "bf16"
    return _lib


def elem_of(dtype):
    """torch dtype a model was moved to -> the build that computes it: float16 -> "fp16"; float32 / bfloat16 -> "bf16"
    (fp32 requests are served by the bf16 build: master parameters stay fp32, compute is bf16 MFMA, fp32 accumulation)."""
    import torch
    return "fp16" if dtype == torch.float16 else "bf16"


def torch_elem(elem):
    import torch
    return torch.float16 if elem == "fp16" else torch.bfloat16


def exported_symbols():
    return sorted(_PROTOS.keys())


def check(rc, what="", l=None):
    """raise on a non-zero return code with the message of the library the call went through: `l`, or the build that lib() handed
    out last (every wrapper fetches its library right before the call)"""
    if rc != 0:
        if l is None:
            l = _lib_f16 if (_last_elem == "fp16" and _lib_f16 is not None) else lib()
        msg = l.dmx_last_error()
        raise RuntimeError(f"diffute_amd: {what} failed (code {rc}): {msg.decode() if msg else ''}")


def poll_device_error(l=None):
    """raise if a kernel of an EARLIER launch gave up on an in-kernel wait (include/diffute_hip.h dmx_device_error): no synchronisation, so
    call it after your own synchronize() to cover the launches in flight"""
    for lb in ([l] if l is not None else [x for x in (_lib, _lib_f16) if x is not None]):
        check(lb.dmx_device_error(), "device error poll", lb)


def exclusive_device(l):
    """current dmx_set_exclusive_device setting of library `l`"""
    return int(l.dmx_get_exclusive_device())


def set_exclusive_device(on):
    """Tell the library (every loaded build) whether its launches have the GPU to themselves (include/diffute_hip.h dmx_set_exclusive_device).
    The default, True, lets dmx_conv3x3_gn split the K range of a tile over co-resident blocks; pass False before running ANYTHING else on the
    same GPU next to the library's launches - a second model on another stream or thread, your own kernels or collectives on a side stream.
    denoise(micro_batches > 1) and set_gradient_sync(world > 1) switch it themselves.  A starved split launch never passes silently: it raises
    DMX_ERR_DEVICE (RuntimeError at the next call, or at diffute_amd.synchronize()).  Returns the previous setting."""
    global _exclusive
    old = True if _exclusive is None else _exclusive
    _exclusive = bool(on)                      # (a build loaded later starts from this setting: _load)
    for lb in (_lib, _lib_f16):
        if lb is not None:
            lb.dmx_set_exclusive_device(1 if on else 0)
    return old


def synchronize(device=None):
    """torch.cuda.synchronize() + the device -> host error poll: the public sync point.  Every launch of the library checks for an error raised by
    an EARLIER launch, so an error inside a sequence of calls surfaces by itself; only the LAST launches before the host reads results
    (the end of denoise(), of a training step, of vae.decode) have nobody after them - synchronise through this function (bench.py, the
    tests and __graft_entry__.smoke() do) and a kernel that gave up on an in-kernel wait raises here instead of handing back a wrong tensor."""
    import torch
    torch.cuda.synchronize(device)
    poll_device_error()


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else c_void_p(t.data_ptr())


def current_stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("diffute_amd: tensors must live on the GPU (cuda / ROCm device); there is no CPU path")
