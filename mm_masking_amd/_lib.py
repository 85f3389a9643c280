"""ctypes binding of libmmk_hip.so (the C ABI declared in include/mmk.h).

This is the stub a maintainer of the reference would add: the
reference has no FFI of its own, so every entry point replaces a *Python* call
site of mm_masking (cited in include/mmk.h).  PyTorch is only the owner of the
device buffers and of the HIP stream the kernels are enqueued on.

Signatures, struct layouts and constants are not written down here: they are
read from include/mmk.h when this module is imported (``read_header``), so the
binding cannot disagree with the declaration.

The library is mandatory: there is NO CPU or PyTorch fallback.  ``lib()`` raises
if the shared object is missing or fails to load, and every wrapper raises if a
tensor is not a contiguous tensor of the expected dtype on a HIP device.
"""
import ctypes
import os
import re
import sys
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
SO_PATH = os.environ.get("MMK_LIB", os.path.join(_HERE, "libmmk_hip.so"))   # MMK_LIB: A/B another build (development)
SOURCES = ["mmk_api.hip", "mmk_icp.hip", "mmk_cloud.hip", "mmk_radar.hip", "mmk_unet.hip", "mmk_unet_driver.hip",
           "mmk_loader.hip", "mmk_loss.hip"]

_lib = None


class MmkError(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------------ include/mmk.h -> ctypes
_SCALARS = {"void": None, "char": ctypes.c_char, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}
_DECLARATION = re.compile(r"typedef\s+struct\s*\w*\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;"
                          r"|(?P<ret>[^;{}()]+?)\((?P<args>[^;{}]*)\)\s*;")


def _ctype(decl, structs, where):
    """(ctypes type, name) of one C declarator such as ``const float *const *params``; a plain ``void`` gives type None.
    ``char *`` is c_char_p, a pointer to a typedef'd struct POINTER(its class), a pointer to a pointer POINTER(c_void_p)
    (it takes a ``(c_void_p * n)`` array both as an argument and as a struct field), every other pointer c_void_p."""
    m = re.fullmatch(r"\s*(\w+)\s*((?:\*\s*)*)(\w*)\s*", re.sub(r"\bconst\b", " ", decl))
    if not m:              # arrays, function pointers, '...', bit-fields, 'unsigned int', 'struct tag': nothing mmk.h uses
        raise MmkError("mmk.h, %s: cannot read the declarator '%s'" % (where, " ".join(decl.split())))
    base, stars, name = m.group(1), m.group(2).count("*"), m.group(3)
    if base not in _SCALARS and base not in structs:
        raise MmkError("mmk.h, %s: unknown type '%s' in '%s' (a struct must be typedef'd above its first use)"
                       % (where, base, " ".join(decl.split())))
    if stars >= 2:
        return ctypes.POINTER(ctypes.c_void_p), name
    if stars == 1:
        return (ctypes.c_char_p if base == "char" else ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p), name
    if base in structs:
        raise MmkError("mmk.h, %s: struct '%s' by value in '%s'" % (where, base, " ".join(decl.split())))
    return _SCALARS[base], name


def read_header(text):
    """The C ABI that the header ``text`` declares, as ctypes: ({function: (restype, [argtypes])}, {typedef name:
    Structure class}, {MMK_* define: int}).  It understands the subset of C that include/mmk.h is written in and raises
    MmkError, naming the declaration, for anything else: a header edit in a new style stops the import instead of
    producing a wrong signature."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", text, flags=re.S)          # the extern "C" brackets
    protos, structs, consts, code = {}, {}, {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(MMK_\w+)[ \t]+(\S.*?)\s*$", line)
        if m:
            value = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", m.group(2))
            if not value:
                raise MmkError("mmk.h, %s: '%s' is not an integer" % (m.group(1), m.group(2)))
            consts[m.group(1)] = int(value.group(1))

    def declare(m):
        if m.group("struct"):
            where, fields = "struct " + m.group("struct"), []
            for member in filter(str.strip, m.group("fields").split(";")):
                first, *more = member.split(",")                      # 'int32_t rows, row_bytes': the type word is shared
                base = re.match(r"(?:\s|\bconst\b)*(\w*)", first).group(1)
                for decl in [first] + [base + " " + d for d in more]:
                    t, field = _ctype(decl, structs, where)
                    if t is None or not field:
                        raise MmkError("mmk.h, %s: cannot read the member '%s'" % (where, " ".join(decl.split())))
                    fields.append((field, t))
            structs[m.group("struct")] = type(m.group("struct"), (ctypes.Structure,),
                                              {"_fields_": fields, "__doc__": "%s of include/mmk.h." % m.group("struct")})
            return " "
        res, name = _ctype(m.group("ret"), structs, "'%s'" % " ".join(m.group("ret").split()))
        args = [] if m.group("args").strip() == "void" else m.group("args").split(",")
        protos[name] = (res, [])
        for decl in args:
            t, arg = _ctype(decl, structs, name)
            if t is None or not arg:
                raise MmkError("mmk.h, %s: parameter '%s' has no %s" % (name, " ".join(decl.split()), "name" if t else "type"))
            protos[name][1].append(t)
        return " "
    rest = _DECLARATION.sub(declare, "\n".join(code)).split()
    if rest:
        raise MmkError("mmk.h: cannot read '%s'" % " ".join(rest[:12]))
    return protos, structs, consts


with open(os.path.join(_ROOT, "include", "mmk.h")) as _f:
    EXPORTED, STRUCTS, CONSTANTS = read_header(_f.read())
IcpParams, IcpSoft, ReadJob, ConvDesc, UNetDesc = (STRUCTS["mmk_" + n] for n in
                                                   ("icp_params", "icp_soft", "read_job", "conv_desc", "unet_desc"))


def _codes(prefix, keys):
    return {k: CONSTANTS[prefix + v] for k, v in keys.items()}


FINAL_BWD_WS_FLOATS = CONSTANTS["MMK_FINAL_BWD_WS_FLOATS"]
NORM_MODES = _codes("MMK_NORM_", {None: "NONE", "none": "NONE", "minmax": "MINMAX", "standardize": "STANDARDIZE"})
ICP_TYPES = _codes("MMK_ICP_", {"pt2pt": "PT2PT", "pt2pl": "PT2PL"})
LOSSES = _codes("MMK_LOSS_", {None: "NONE", "none": "NONE", "l2": "NONE", "cauchy": "CAUCHY", "huber": "HUBER",
                              "geman_mcclure": "GEMAN_MCCLURE", "welsch": "WELSCH"})
NN_METHODS = _codes("MMK_NN_", {"brute": "BRUTE", "grid": "GRID"})
VOXEL_MODES = _codes("MMK_VOXEL_", {"centroid": "CENTROID", "first": "FIRST"})


def build(verbose=False):
    """Compile the HIP sources for gfx950 into mm_masking_amd/libmmk_hip.so (hipcc cross-compiles without a GPU): one
    object per source (in parallel, only the stale ones), then one link.  -ffp-contract=off is part of the numerical
    contract."""
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, s) for s in SOURCES]
    common = [os.path.join(csrc, "mmk_common.h"), os.path.join(csrc, "mmk_unet_shared.h"), os.path.join(_ROOT, "include", "mmk.h")]
    incs = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith(".inc")]
    extra = {"mmk_unet.hip": incs, "mmk_loader.hip": incs}
    objdir = os.path.join(csrc, "_obj")
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", os.path.join(_ROOT, "include")]
    # mmk_unet.hip: MFMA results in VGPRs instead of AGPRs.  The thin-layer kernels are bound by vector-instruction issue and the
    # compiler's default parks their accumulators in AGPRs, which vector instructions cannot read: every output value then costs
    # a v_accvgpr_read (4 184 of them in the file, 96 with the option; same arithmetic, same or better occupancy; HISTORY.md 10.17)
    per_file = {"mmk_unet.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        deps = [src] + common + extra.get(os.path.basename(src), []) + [os.path.abspath(__file__)]
        if not (os.path.exists(obj) and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in deps)):
            jobs.append([hipcc] + flags + per_file.get(os.path.basename(src), []) + ["-c", src, "-o", obj])
    if not jobs and os.path.exists(SO_PATH) and all(os.path.getmtime(SO_PATH) >= os.path.getmtime(o) for o in objs):
        return SO_PATH

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        try:
            subprocess.check_call(cmd)
        except subprocess.CalledProcessError:
            # a hipcc that does not know a backend option of per_file: same code without it (slower kernels, same results)
            plain = [c for c in cmd if c not in sum(per_file.values(), [])]
            if len(plain) == len(cmd):
                raise
            print("libmmk_hip: retrying without %s" % " ".join(sorted(set(cmd) - set(plain))), file=sys.stderr, flush=True)
            subprocess.check_call(plain)
    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO_PATH] + objs)
    return SO_PATH


def _declare(lib):
    for name, (res, args) in EXPORTED.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def lib():
    """The loaded C-ABI library; raises MmkError when it is absent (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise MmkError("libmmk_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  The HIP path has no CPU fallback.")
        try:
            loaded = ctypes.CDLL(SO_PATH)
        except OSError as e:
            raise MmkError("cannot load %s: %s" % (SO_PATH, e)) from e
        _declare(loaded)
        if loaded.mmk_conv_desc_bytes() != ctypes.sizeof(ConvDesc):
            raise MmkError("%s: mmk_conv_desc is %d bytes, the ctypes class %d" % (SO_PATH, loaded.mmk_conv_desc_bytes(), ctypes.sizeof(ConvDesc)))
        if loaded.mmk_icp_params_bytes() != ctypes.sizeof(IcpParams):
            raise MmkError("%s: mmk_icp_params is %d bytes, the ctypes class %d" % (SO_PATH, loaded.mmk_icp_params_bytes(), ctypes.sizeof(IcpParams)))
        _lib = loaded
    return _lib


def check(rc):
    if rc != 0:
        raise MmkError("libmmk_hip: %s (code %d)" % (lib().mmk_last_error().decode(errors="replace"), rc))


def stream_ptr(device=None):
    """The current PyTorch HIP stream of ``device`` as a void*.  The C entry points launch on the calling
    thread's *current* HIP device (include/mmk.h), so a tensor that lives on another device than the
    current one would meet a foreign stream handle: refuse that instead of faulting."""
    if device is not None:
        idx = device.index if isinstance(device, torch.device) else int(device)
        if idx is not None and idx != torch.cuda.current_device():
            raise MmkError("tensors live on cuda:%d but the current HIP device is cuda:%d: call torch.cuda.set_device() "
                           "(one process per GPU) or wrap the call in `with torch.cuda.device(...)`"
                           % (idx, torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t, dtype=None, name="tensor"):
    """Device pointer of a contiguous HIP tensor (None -> NULL)."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise MmkError("%s must live on a HIP device (got %s); the kernels have no CPU path" % (name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise MmkError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise MmkError("%s must be contiguous" % name)
    return ctypes.c_void_p(t.data_ptr())


_ws_cache = {}


def workspace(nbytes, device, tag):
    """Scratch of at least ``nbytes`` for the kernels of one family (``tag``: callers under different tags never share a
    buffer), one growing buffer per (device, stream, tag): calls enqueued on different streams must not share scratch."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def dev_f32(t, device):
    """Reference call sites hand over CPU or device tensors of any float type
    (icp_weight_policy.py:130-134 moves them itself); normalise to contiguous
    fp32 on `device`."""
    return t.detach().to(device=device, dtype=torch.float32).contiguous()
