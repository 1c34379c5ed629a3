"""ctypes binding of libvexpress_hip.so (C ABI: include/vexpress_hip.h and, for the guidance and sampler entry points added
after it, include/vexpress_hip_guidance.h, include/vexpress_hip_samplers.h, include/vexpress_hip_solvers.h,
include/vexpress_hip_reuse.h and include/vexpress_hip_resize.h).

There is NO fallback: if the library is missing, unbuildable or lacks a symbol, importing this module
raises.  The library is built in-tree (v-express_amd/libvexpress_hip.so) by `__graft_entry__.build()` /
`make -C v-express_amd/csrc`, so it travels with the repo snapshot to the GPU box.
"""
import ctypes as C
import os
import subprocess

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# VX_LIBRARY: another build of the SAME library (same-box A/B runs of kernel variants, tools/ only); default in-tree
LIB_PATH = os.environ.get("VX_LIBRARY") or os.path.join(_HERE, "libvexpress_hip.so")
CSRC = os.path.join(_HERE, "csrc")
HEADER = abi.HEADER
GUIDANCE_HEADER = abi.GUIDANCE_HEADER
SAMPLERS_HEADER = abi.SAMPLERS_HEADER
SOLVERS_HEADER = abi.SOLVERS_HEADER
REUSE_HEADER = abi.REUSE_HEADER
RESIZE_HEADER = abi.RESIZE_HEADER

# the binding is DERIVED from the header (abi.py reads it once per process): the enum constants, the ctypes mirrors of the
# four parameter structs and, in _load, argtypes / restype of every function - there is no second copy to keep in step
globals().update(abi.header().enums)                 # VX_EPI_*, VX_PART_*, VX_ACT_*
GemmParams, FfParams, TBlockParams, AxAttnParams = (
    abi.header().classes[s] for s in ("vx_gemm_params", "vx_ff_params", "vx_tblock_params", "vx_axattn_params"))


def declared_symbols():
    """Every function name declared in include/vexpress_hip.h."""
    return sorted(abi.header().functions)


def build(force=False):
    """Compile the HIP sources for gfx950 (cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    r = subprocess.run(["make", "-C", CSRC, "-j", str(os.cpu_count() or 4)], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(LIB_PATH):
        raise RuntimeError("building libvexpress_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def _load(path=None, element="bf16"):
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C v-express_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(path)
    # the six headers, each with its own version: the first one's, then the guidance, sampler, solver, guidance-reuse
    # and latent-resize entry points
    for hdr, version in ((abi.header(), "vx_abi_version"), (abi.guidance_header(), "vx_guidance_abi_version"),
                         (abi.samplers_header(), "vx_samplers_abi_version"),
                         (abi.solvers_header(), "vx_solvers_abi_version"),
                         (abi.reuse_header(), "vx_reuse_abi_version"),
                         (abi.resize_header(), "vx_resize_abi_version")):
        missing = [s for s in sorted(hdr.functions) if not hasattr(lib, s)]
        if missing:
            raise ImportError(f"{path} does not export {missing}; rebuild it")
        for name, (restype, params) in hdr.functions.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, [ctype for _, ctype in params]
        if getattr(lib, version)() != hdr.version:
            raise ImportError(f"{os.path.basename(path)} ABI version mismatch ({version})")
    if lib.vx_element_type().decode() != element:
        raise ImportError(f"{path} computes on {lib.vx_element_type().decode()} elements, expected {element}")
    return lib


lib = _load()

# ---- the element type of the running computation.  libvexpress_hip.so computes on bfloat16 storage, libvexpress_hip_f16.so
# (the same sources, -DVX_ELEM_F16, the same ABI) on IEEE half - the reference's default `--dtype fp16`
# (inference.py:44,150-151).  Which one a call goes to is decided by the MODEL's dtype: every model entry point runs inside
# `with element_type(model element)` (module_base.DeviceModule), ops.py allocates in ELEM[0] and calls `current()`.
import torch  # noqa: E402

LIB16_PATH = os.environ.get("VX_LIBRARY_F16") or os.path.join(_HERE, "libvexpress_hip_f16.so")
ELEM = [torch.bfloat16]
_LIB16 = [None]


def lib_f16():
    """The IEEE-half build, loaded on first use (a missing / stale / mismatching library is an ImportError, like the bf16 one)."""
    if _LIB16[0] is None:
        l16 = _load(LIB16_PATH, "f16")
        if not os.environ.get("VX_LIBRARY_F16") and not os.environ.get("VX_LIBRARY"):
            a, b = l16.vx_build_id().decode(), lib.vx_build_id().decode()
            if a != b:
                raise ImportError(f"{LIB16_PATH} ({a}) and {LIB_PATH} ({b}) were built from different sources: rebuild both")
        _LIB16[0] = l16
    return _LIB16[0]


def current():
    """The library of the element type in force (ELEM[0])."""
    return lib if ELEM[0] is torch.bfloat16 else lib_f16()


class element_type:
    """`with element_type(torch.float16):` - calls and allocations of ops.py inside the block use the IEEE-half library."""

    def __init__(self, dtype):
        if dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"the kernels compute on bfloat16 or float16 elements, not {dtype}")
        self.dtype = dtype

    def __enter__(self):
        self.prev = ELEM[0]
        ELEM[0] = self.dtype
        if self.dtype is torch.float16:
            lib_f16()
        return self

    def __exit__(self, *a):
        ELEM[0] = self.prev


def source_id():
    """sha256 (first 16 hex digits) over the kernel sources the library is built from - csrc/*.hip / *.h / *.cpp and the
    six C ABI headers, in name order.  (Of the sources, not of the .so: a rebuild on another machine need not be
    byte-identical, the sources it was built from are.  tools/lib_id.py prints the same value without importing torch.)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) +
                   glob.glob(os.path.join(CSRC, "*.cpp")) + [os.path.join(CSRC, "Makefile"), HEADER, GUIDANCE_HEADER,
                                                              SAMPLERS_HEADER, SOLVERS_HEADER, REUSE_HEADER,
                                                              RESIZE_HEADER])
    try:
        for path in files:
            h.update(os.path.basename(path).encode())
            with open(path, "rb") as f:
                h.update(f.read())
    except OSError:
        return None                      # a binary-only install: nothing to compare the library with
    return h.hexdigest()[:16]


def _build_identity():
    """Identity of the LOADED binary: `vx_build_id()` = "<source hash the Makefile stamped>|<extra -D flags>".
    * stamped, no extra flags, hash == the sources on disk: that hash (what committed profiles are keyed by);
    * stamped with extra -D flags (make EXTRA_DEFS=...): "<hash>+<flags>" - never equal to a plain hash;
    * loaded through VX_LIBRARY (A/B builds of tools/build_*_variants.sh): "variant:<file name>"; unstamped: "unstamped:<file name>";
    * stamped with ANOTHER hash than the sources on disk: the .so is stale -> ImportError (VX_ALLOW_STALE_LIB=1: a warning
      and the identity "stale:<hash>", so that no committed measurement is paired with it)."""
    src, _, defs = lib.vx_build_id().decode().partition("|")
    if os.environ.get("VX_LIBRARY"):
        # an explicitly chosen A/B build (tools/build_*_variants.sh link the product's stamped vx_api.o): never the product
        return "variant:" + os.path.basename(LIB_PATH)
    if src == "unstamped" or len(src) != 16 or any(ch not in "0123456789abcdef" for ch in src):
        # (an empty or malformed stamp - tools/lib_id.py failed inside make - is "unstamped" too, never "stale": ADVICE r05)
        return "unstamped:" + os.path.basename(LIB_PATH)
    disk = source_id()
    if disk is not None and disk != src:
        msg = (f"{LIB_PATH} was built from kernel sources {src}, the sources on disk are {disk}: rebuild it "
               "(make -C v-express_amd/csrc, or __graft_entry__.build())")
        if os.environ.get("VX_ALLOW_STALE_LIB") != "1":
            raise ImportError(msg)
        import warnings
        warnings.warn(msg)
        return "stale:" + src
    return src + ("+" + defs if defs else "")


# identity of the kernel build: measurements committed under profiles/ carry it, and bench.py quotes a committed trace /
# counter file next to a live number only when it was taken with the SAME binary (`vx_build_id`, stamped by the Makefile)
LIB_SHA256 = _build_identity()


class VxError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        msg = current().vx_last_error_string().decode("utf-8", "replace")
        raise VxError(f"libvexpress_hip {what} failed (rc={rc}): {msg}")
