"""The C-ABI library loads without a GPU and exports every function include/ocppo.h declares;
argument validation and the error channel work without launching anything."""
import ctypes
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from oc_cleanrl_amd import _lib

    return _lib


def test_header_functions_exported(lib):
    names = lib.header_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib.LIB, n), f"{n} declared in include/ocppo.h but not exported"
        assert n in lib.SIGNATURES, f"{n} has no ctypes signature"
    assert set(lib.SIGNATURES) == set(names)


def test_header_constants_match_python(lib):
    text = (ROOT / "include" / "ocppo.h").read_text()
    consts = dict(re.findall(r"#define (OCPPO_\w+) (\d+)", text))
    assert int(consts["OCPPO_ABI_VERSION"]) == lib.OCPPO_ABI_VERSION == lib.LIB.ocppo_abi_version()
    assert int(consts["OCPPO_F32"]) == lib.OCPPO_F32
    assert int(consts["OCPPO_BF16"]) == lib.OCPPO_BF16
    assert int(consts["OCPPO_U8"]) == lib.OCPPO_U8
    assert int(consts["OCPPO_NUM_STATS"]) == lib.OCPPO_NUM_STATS
    stat_names = re.findall(r"#define OCPPO_STAT_(\w+) (\d+)", text)
    assert [n.lower() for n, _ in sorted(stat_names, key=lambda x: int(x[1]))] == list(lib.STAT_NAMES)


SYNTHETIC_HEADER = """
/* a comment with a call in it: ocppo_ghost(int x); and an unbalanced ( too */
#ifndef OCPPO_H
#define OCPPO_H
#define OCPPO_ABI_VERSION 7
#define OCPPO_STAT_B 1 /* second (by value) */
#define OCPPO_STAT_A 0 // first: ocppo_other(
#define OCPPO_NOT_DECIMAL 0x10
#define OCPPO_API __attribute__((visibility("default")))
typedef void* ocppo_stream_t; /* hipStream_t */
OCPPO_API int ocppo_version(void);
OCPPO_API const char* ocppo_message(void);
// OCPPO_API int ocppo_commented_out(int x);
OCPPO_API int ocppo_many(ocppo_stream_t stream, const float* const* src,  /* ( */
                         void* const* dst, float scale,
                         uint32_t seed, int64_t n,
                         uint64_t key, double lr, size_t bytes, int flag);
OCPPO_API size_t ocppo_bytes(int64_t n);
OCPPO_API int64_t
ocppo_chunks(int64_t n);
#endif
"""


def test_parse_header_on_synthetic_text(lib):
    c = ctypes
    sigs, consts = lib.parse_header(SYNTHETIC_HEADER)
    assert sigs == {
        "ocppo_version": (c.c_int, []),
        "ocppo_message": (c.c_char_p, []),
        "ocppo_many": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_float, c.c_uint32,
                                 c.c_int64, c.c_uint64, c.c_double, c.c_size_t, c.c_int]),
        "ocppo_bytes": (c.c_size_t, [c.c_int64]),
        "ocppo_chunks": (c.c_int64, [c.c_int64]),
    }
    assert consts == {"OCPPO_ABI_VERSION": 7, "OCPPO_STAT_B": 1, "OCPPO_STAT_A": 0}


@pytest.mark.parametrize("decl, names", [
    ("OCPPO_API int ocppo_f(const float* x, long count);", ("ocppo_f", "count")),  # unknown scalar
    ("OCPPO_API int ocppo_f(unsigned int count);", ("ocppo_f", "count")),
    ("OCPPO_API int ocppo_f(ocppo_deferred_finish_t rec);", ("ocppo_f", "rec")),  # struct by value
    ("OCPPO_API int ocppo_f(int64_t n, float taps[4]);", ("ocppo_f", "taps")),  # array
    ("OCPPO_API int ocppo_f(float taps[]);", ("ocppo_f", "taps")),
    ("OCPPO_API int ocppo_f(void (*done)(int));", ("ocppo_f", "done")),  # function pointer
    ("OCPPO_API int ocppo_f(int64_t);", ("ocppo_f", "int64_t")),  # unnamed parameter
    ("OCPPO_API void ocppo_f(int64_t n);", ("ocppo_f", "return")),  # no status to check
    ("OCPPO_API long ocppo_f(int64_t n);", ("ocppo_f", "return")),
])
def test_parse_header_refuses_what_it_cannot_map(lib, decl, names):
    with pytest.raises(ImportError) as e:
        lib.parse_header(decl)
    for n in names:
        assert n in str(e.value)


def test_parse_header_refuses_a_declaration_it_cannot_read(lib):
    with pytest.raises(ImportError):
        lib.parse_header("OCPPO_API int (*ocppo_f(int64_t n))(int);")
    with pytest.raises(ImportError):  # a name declared twice
        lib.parse_header("OCPPO_API int ocppo_f(int64_t n);\nOCPPO_API int ocppo_f(int n);")


def test_pinned_signatures(lib):
    """Literal copies of the hand-typed table this binding once held, for entries that between
    them use every mapped type: the parser must keep deriving exactly these."""
    P, I64, U64, D, I, SZ = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double,
                             ctypes.c_int, ctypes.c_size_t)
    U32, F = ctypes.c_uint32, ctypes.c_float
    pinned = {
        "ocppo_last_error": (ctypes.c_char_p, []),
        "ocppo_ppo_loss_workspace_bytes": (SZ, [I64, I64]),
        "ocppo_gae": (I, [P, P, P, P, P, P, I64, I64, D, D, P, P]),
        "ocppo_dropout": (I, [P, P, P, I64, U32, F, I64, P]),
        "ocppo_conv_x6_u8": (I, [P, I, P, P, I64, I64, I64, I64, I64, I64, P, I64, P, I64, I64,
                                 I64, I64, P, I, F, I, P, P, P, P]),
        "ocppo_polyak": (I, [P, I, P, P, P, D]),
        "ocppo_deferred_finish_run": (I, [P, P]),
        "ocppo_relu_bias_grad_chunks": (I64, [I64, I64]),
        "ocppo_replay_sample": (I, [P, U64, P, P, I64, I64, I64, P, I, P, P, P, I64, P, P, P, P,
                                    P, P]),
    }
    for name, (restype, argtypes) in pinned.items():
        assert lib.SIGNATURES[name] == (restype, argtypes), name
        fn = getattr(lib.LIB, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    used = {t for r, a in pinned.values() for t in [r, *a]}
    assert used == {t for r, a in lib.SIGNATURES.values() for t in [r, *a]}


def test_header_defines_are_module_constants(lib):
    text = (ROOT / "include" / "ocppo.h").read_text()
    consts = dict(re.findall(r"#define (OCPPO_\w+) (\d+)", text))
    assert len(consts) >= 30
    for name, value in consts.items():
        assert getattr(lib, name) == int(value), name
    from oc_cleanrl_amd import ops

    assert (ops.OPT_STEP, ops.OPT_TOTAL_NORM, ops.OPT_CLIP_COEF, ops.OPT_TAIL_SKIPPED,
            ops.OPT_TAIL_STEP) == (0, 1, 2, 6, 7)  # the header's values at ABI 43


def test_call_sites_name_declared_entry_points(lib):
    """Every entry point the package names -- a string literal (passed to call( directly, chosen
    by a conditional, or kept as a class's ENTRY) or an attribute of LIB -- is declared in the
    header: a typo in a rarely-taken path fails here, not on a GPU. Only a by-name
    getattr(LIB, "...") is left out: that is how a probe build's symbol outside the C-ABI is
    reached."""
    named = {}
    for src in sorted((ROOT / "oc_cleanrl_amd").glob("*.py")):
        text = src.read_text()
        pattern = r"\bLIB\.(ocppo_\w+)"
        if src.name != "_lib.py":  # (whose string literals are the parser's type names)
            pattern += r"|(?<!LIB, )[\"'](ocppo_\w+)[\"']"
        for m in re.finditer(pattern, text):
            named.setdefault(m.group(m.lastindex), src.name)
    assert len(named) >= 100 and "ocppo_clip_radam_step" in named
    unknown = {n: f for n, f in named.items() if n not in lib.SIGNATURES}
    assert not unknown, unknown


def test_only_c_abi_is_exported():
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only",
                          str(ROOT / "oc_cleanrl_amd" / "lib" / "libocppo_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = [l.split()[-1] for l in out.splitlines() if l.split()[1] in ("T", "D", "B", "W", "V")]
    assert all(s.startswith("ocppo_") for s in syms), [s for s in syms if not s.startswith("ocppo_")]


def test_invalid_arguments_report_errors_without_launch(lib):
    L = lib.LIB
    rc = L.ocppo_gae(None, None, None, None, None, None, 8, 4, 0.99, 0.95, None, None)
    assert rc == lib.OCPPO_E_INVALID
    assert b"null pointer" in L.ocppo_last_error()
    rc = L.ocppo_ppo_loss_fwd_bwd(None, None, None, 16, 64, *([None] * 7), 0.1, 0.01, 0.5, 1, 1,
                                  None, None, None, None, 0)
    assert rc == lib.OCPPO_E_INVALID and b"A <= 32" in L.ocppo_last_error()
    dummy = ctypes.c_void_p(16)
    rc = L.ocppo_ppo_loss_fwd_bwd(None, dummy, dummy, 16, 6, None, dummy, dummy, dummy, dummy,
                                  dummy, None, 0.1, 0.01, 0.5, 1, 1, dummy, dummy, dummy, None, 0)
    assert rc == lib.OCPPO_E_WORKSPACE
    with pytest.raises(lib.OcppoError, match="ocppo_gather_rows"):
        lib.call("ocppo_gather_rows", None, None, 7, None, 4, 4, None)


def test_deferred_finish_record_is_checked(lib):
    """ocppo_deferred_finish_run / ocppo_sum_splits_finish refuse a missing record or one no
    ocppo_heads_loss_rows call filled, before any launch."""
    L = lib.LIB
    assert L.ocppo_deferred_finish_run(None, None) == lib.OCPPO_E_INVALID
    assert b"null finish record" in L.ocppo_last_error()
    rec = (ctypes.c_uint64 * 64)()
    assert L.ocppo_deferred_finish_run(None, ctypes.addressof(rec)) == lib.OCPPO_E_INVALID
    assert b"not a finish record" in L.ocppo_last_error()
    dummy = ctypes.c_void_p(256)
    assert L.ocppo_sum_splits_finish(None, dummy, 8, 1024, dummy,
                                     ctypes.addressof(rec)) == lib.OCPPO_E_INVALID
    assert b"not a finish record" in L.ocppo_last_error()
    assert L.ocppo_sum_splits_finish(None, dummy, 3, 1024, dummy,
                                     ctypes.addressof(rec)) == lib.OCPPO_E_INVALID
    assert b"bad sizes" in L.ocppo_last_error()


def test_zero_sized_calls_are_noops(lib):
    assert lib.LIB.ocppo_gae(None, None, None, None, None, None, 0, 0, 0.99, 0.95, None, None) == 0
    assert lib.LIB.ocppo_gather_rows(None, None, 0, None, 0, 4, None) == 0


def test_workspace_size_is_host_only(lib):
    n = lib.LIB.ocppo_ppo_loss_workspace_bytes(4096, 6)
    assert n >= 256 + 16 * 6 * 4 and n % 16 == 0


def test_library_reads_no_environment():
    """No tiling, grid or workspace choice of the shipped library depends on the environment:
    it imports no getenv (the geometry knobs of experiments are compile-time -D flags for
    tools/build_variant.py, or explicit ABI arguments such as ocppo_gemm_x6's mbig)."""
    import subprocess

    out = subprocess.run(["nm", "-D", "--undefined-only",
                          str(ROOT / "oc_cleanrl_amd" / "lib" / "libocppo_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    assert not [l for l in out.splitlines() if "getenv" in l]
    for src in (ROOT / "oc_cleanrl_amd" / "csrc").glob("*.hip"):
        assert "getenv" not in src.read_text(), src.name


def test_gemm_x6_mbig_only_for_the_mixed_tile(lib):
    dummy = ctypes.c_void_p(256)
    args = [None, dummy, 64, 1, dummy, 64, 1, dummy, 128, 128, 128, 64, 1, 0, None, 0, None, 0,
            None, None, None]
    assert lib.LIB.ocppo_gemm_x6(*args, 24, 512, None, 0, 0, None, 0) == lib.OCPPO_E_INVALID
    assert b"mbig" in lib.LIB.ocppo_last_error()


def test_gemm_x6_rejects_operand_windows_past_32_bit_offsets(lib):
    """The x6 kernels address a tile's operand window with 32-bit buffer offsets: a row stride
    that puts one 128-row window past 2 GiB is refused before any launch (validation only)."""
    dummy = ctypes.c_void_p(256)
    ok = [None, dummy, 64, 1, dummy, 64, 1, dummy, 128, 128, 128, 64, 1, 0, None, 0, None, 0,
          None, None, None, 24, -1, None, 0, 0, None, 0]
    big = list(ok)
    big[2] = 1 << 22  # A row stride 4M floats: 256 rows x 16 MB
    assert lib.LIB.ocppo_gemm_x6(*big) == lib.OCPPO_E_INVALID
    assert b"2 GiB" in lib.LIB.ocppo_last_error()
