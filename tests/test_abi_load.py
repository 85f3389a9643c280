"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol
that include/mmk.h declares (no compute calls without a GPU); the binding that
_lib derives from the header (arity, struct layout against the C compiler,
constants, refusal of declarations it does not understand); host-side argument
checking; the product fails loudly instead of falling back when no GPU exists."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

from mm_masking_amd import _lib
from support import header, n_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_header_symbols_exported(L):
    hdr = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(mmk_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 15
    for n in sorted(names):
        assert hasattr(L, n), "symbol %s declared in mmk.h is not exported" % n
    assert names == set(_lib.EXPORTED.keys()), names ^ set(_lib.EXPORTED.keys())
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmk.h")).read()
    assert L.mmk_version() == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", hdr).group(1))


def test_arity_of_every_entry():
    """Every derived signature has as many arguments as the header declares, counted by support.n_args, which shares no
    code with the reader of _lib."""
    hdr = header()
    assert len(_lib.EXPORTED) >= 119
    for name, (_, argtypes) in _lib.EXPORTED.items():
        assert len(argtypes) == n_args(hdr, name), name


def test_struct_layout_against_the_c_compiler(tmp_path):
    """sizeof and every offsetof as the host C compiler lays out the header's structs == the ctypes classes."""
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler (cc) on this machine")
    names = set(re.findall(r"\}\s*(\w+)\s*;", header()))
    assert names == set(_lib.STRUCTS) and len(names) >= 5
    for py, c in (("IcpParams", "mmk_icp_params"), ("IcpSoft", "mmk_icp_soft"), ("ReadJob", "mmk_read_job"),
                  ("ConvDesc", "mmk_conv_desc"), ("UNetDesc", "mmk_unet_desc")):
        assert getattr(_lib, py) is _lib.STRUCTS[c]
    want, lines = [], []
    for s, cls in sorted(_lib.STRUCTS.items()):
        want.append("%s %d" % (s, ctypes.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in cls._fields_:
            want.append("%s.%s %d %d" % (s, f, getattr(cls, f).offset, getattr(cls, f).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "mmk.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    assert subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")[:-1] == want


@pytest.mark.parametrize("text, names", [
    ("int mmk_f(long n);", "mmk_f.*long"),                                          # an unknown type word
    ("int mmk_f(unsigned int n);", "mmk_f.*unsigned int n"),
    ("int mmk_f(float v[3]);", r"mmk_f.*v\[3\]"),                                    # an array parameter
    ("int mmk_f(int32_t n, void (*cb)(int));", "mmk_f.*cb"),                         # a function-pointer parameter
    ("int mmk_f(const char *fmt, ...);", r"mmk_f.*\.\.\."),
    ("typedef struct { int32_t a; } mmk_s;\nint mmk_f(mmk_s s);", "mmk_f.*mmk_s.*by value"),
    ("typedef struct { int32_t a; } mmk_s;\nmmk_s mmk_f(void);", "mmk_s.*by value"),
    ("int mmk_f(const mmk_t *p);\ntypedef struct { int32_t a; } mmk_t;", "mmk_f.*mmk_t"),   # not typedef'd yet
    ("int mmk_f(int32_t);", "mmk_f.*int32_t.*name"),                                 # an unnamed parameter
    ("int mmk_f();", "mmk_f"),
    ("typedef struct { int32_t a : 3; } mmk_s;", "mmk_s.*a : 3"),                    # a bit-field
    ("typedef struct { float v[4]; } mmk_s;", r"mmk_s.*v\[4\]"),
    ("typedef struct { struct { int32_t a; } in; } mmk_s;", "typedef struct"),
    ("typedef int32_t mmk_i;", "typedef int32_t mmk_i"),
    ("enum mmk_e { MMK_A };", "enum mmk_e"),
    ("#define MMK_N (1 << 4)", "MMK_N.*1 << 4"),
    ("#define MMK_X 1.5f", "MMK_X.*1.5f"),
])
def test_reader_refuses_what_it_does_not_understand(text, names):
    with pytest.raises(_lib.MmkError, match=names):
        _lib.read_header(text)


def test_reader_on_one_declaration_of_each_kind():
    protos, structs, consts = _lib.read_header("""
        /* a comment with int mmk_not_a_function(void); inside */
        #ifndef MMK_H_
        #define MMK_H_
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define MMK_A 7 /* trailing comment */
        #define MMK_B (-3)
        #define MMK_C (12)
        #define OTHER 1
        typedef struct mmk_tag {
            const char *path;
            int32_t rows, cols;
            const float *x, y;
            const float *const *params;
            void *const *outs;
            size_t n; uint64_t key; double d; char c;
        } mmk_s;
        int mmk_none(void);
        const char *mmk_text(const char *path, char c);
        size_t mmk_scalars(int a, int32_t b, int64_t c, uint32_t d, uint64_t e, size_t f, float g,
                           double h);
        int32_t mmk_pointers(const mmk_s *s, mmk_s *t, const float *x, void *y, const int32_t *z, int *n, const uint64_t *k,
                             float *const *grads, void *const *events);
        void mmk_nothing(void *stream);
        void *mmk_handle(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    c = ctypes
    assert consts == {"MMK_A": 7, "MMK_B": -3, "MMK_C": 12}
    S = structs["mmk_s"]
    assert list(structs) == ["mmk_s"] and issubclass(S, c.Structure)
    assert S._fields_ == [("path", c.c_char_p), ("rows", c.c_int32), ("cols", c.c_int32), ("x", c.c_void_p), ("y", c.c_float),
                          ("params", c.POINTER(c.c_void_p)), ("outs", c.POINTER(c.c_void_p)), ("n", c.c_size_t),
                          ("key", c.c_uint64), ("d", c.c_double), ("c", c.c_char)]
    arr = (c.c_void_p * 2)(5, 6)
    s = S(rows=3, params=arr)                             # a T *const * member takes an array of pointers
    assert (s.rows, s.cols, s.path, s.x, s.params[1]) == (3, 0, None, None, 6)
    assert protos == {
        "mmk_none": (c.c_int, []),
        "mmk_text": (c.c_char_p, [c.c_char_p, c.c_char]),
        "mmk_scalars": (c.c_size_t, [c.c_int, c.c_int32, c.c_int64, c.c_uint32, c.c_uint64, c.c_size_t, c.c_float, c.c_double]),
        "mmk_pointers": (c.c_int32, [c.POINTER(S), c.POINTER(S)] + [c.c_void_p] * 5 + [c.POINTER(c.c_void_p)] * 2),
        "mmk_nothing": (None, [c.c_void_p]),
        "mmk_handle": (c.c_void_p, []),
    }


def test_constants_come_from_the_header():
    raw = open(os.path.join(ROOT, "include", "mmk.h")).read()
    defines = {n: int(v) for n, v in re.findall(r"^#define\s+(MMK_\w+)\s+\(?(-?\d+)\)?", raw, flags=re.M)}
    assert len(defines) >= 21 and defines == _lib.CONSTANTS
    assert _lib.CONSTANTS["MMK_VERSION"] == 502 and _lib.CONSTANTS["MMK_ERR_WORKSPACE"] == -3
    assert _lib.FINAL_BWD_WS_FLOATS == 16384
    assert _lib.NORM_MODES == {None: 0, "none": 0, "minmax": 1, "standardize": 2}
    assert _lib.ICP_TYPES == {"pt2pt": 0, "pt2pl": 1}
    assert _lib.LOSSES == {None: 0, "none": 0, "l2": 0, "cauchy": 1, "huber": 2, "geman_mcclure": 3, "welsch": 4}
    assert _lib.NN_METHODS == {"brute": 0, "grid": 1}
    icp_mod = importlib.import_module("mm_masking_amd.dICP.ICP")        # (the package re-exports the class under the module's name)
    assert (icp_mod.ICP_STATUS_UNARMED_KEY, icp_mod.ICP_STATUS_BAD_HYPER) == (1, 2)


def test_host_side_argument_checks(L):
    p = _lib.IcpParams(B=2, N=100, M=300, tgt_cols=6, dim=2, icp_type=1, loss=2, loss_k=1.0, trim_dist=5.0,
                       tolerance=1e-5, max_iter=10, save_state=1, check_every=0, nn_method=0)
    need = L.mmk_icp_workspace_bytes(ctypes.byref(p))
    assert need > 2 * 2 * 1024 * 4
    assert L.mmk_nn_padded_m(20000) == 20480 and L.mmk_nn_padded_m(1) == 1024
    assert L.mmk_nn_workspace_bytes(32, 5120, 20000, 2) >= 2 * 32 * 5120 * 4
    bad = _lib.IcpParams(B=2, N=100, M=300, tgt_cols=3, dim=2, icp_type=1, loss=2, loss_k=1.0, trim_dist=5.0,
                         tolerance=1e-5, max_iter=10, save_state=1, check_every=0, nn_method=0)
    assert L.mmk_icp_workspace_bytes(ctypes.byref(bad)) == 0
    assert b"normals" in L.mmk_last_error()
    bad.tgt_cols, bad.dim = 6, 4
    assert L.mmk_icp_workspace_bytes(ctypes.byref(bad)) == 0 and b"dim" in L.mmk_last_error()
    bad.dim, bad.nn_method = 2, 7
    assert L.mmk_icp_workspace_bytes(ctypes.byref(bad)) == 0 and b"nn_method" in L.mmk_last_error()
    p.nn_method = 1
    assert L.mmk_icp_workspace_bytes(ctypes.byref(p)) > need      # the grid engine carves its cell tables
    null = ctypes.c_void_p(0)
    assert L.mmk_cfar_mask(null, 1, 1, 1, 50, 5, 56, 1, 1.0, 0.09, 0, 10.0, null, null) == -1
    assert L.mmk_nn_search(null, null, null, 1, 1, 1, 2, null, null, null, 0, null) == -1
    assert L.mmk_bev_raster(null, 1, 1, 6, 640, 0.2384, null, null) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU error path")
def test_no_cpu_fallback():
    from mm_masking_amd import radar_utils as ru
    from mm_masking_amd.dICP.ICP import ICP
    with pytest.raises(_lib.MmkError):
        ru.cfar_mask(torch.zeros(1, 4, 400), 0.0596)
    with pytest.raises(_lib.MmkError):
        ru.extract_weights(torch.zeros(1, 640, 640), torch.zeros(1, 4, 3))
    with pytest.raises(_lib.MmkError):
        ICP("pt2pt").icp(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), dim=2)
    icp = ICP(icp_type="pt2pl", config_path="../external/dICP/config/dICP_config.yaml")
    assert icp.target_pad_val == 1000.0


def test_product_does_not_import_oracle():
    import subprocess
    import sys
    code = ("import sys; import mm_masking_amd.train_icp_weights, mm_masking_amd.radar_utils, "
            "mm_masking_amd.icp_weight_policy, mm_masking_amd.dICP.ICP; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
    for root, _, files in os.walk(os.path.join(ROOT, "mm_masking_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(root, f)).read()
                assert "from oracle" not in txt and "import oracle" not in txt, f

