"""CPU: the ctypes binding and the shared limits are derived from include/nsid.h (neuralsampleid_amd/_lib.py parse_header); no
compute calls."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(libpath):
    from neuralsampleid_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def libpath():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


def protos(L, text):
    return L.parse_header(text)[0]


# ---- the parser on small synthetic headers

def test_multi_line_prototype_and_comment_inside_the_arguments(L):
    text = """/* a block
    comment with nsid_not_a_function( in it */
    int nsid_a(const void* x, int ldx,
               float* out /* of x
                             and more */, int act_dtype /* of x and out */,
               void* stream);
    """
    assert protos(L, text) == {"nsid_a": ("i", "pipis")}


def test_void_and_return_types(L):
    text = "int nsid_a(void);\nlong nsid_b(void);\nsize_t nsid_c(int Bg);\nconst char* nsid_d(int i);\nconst char *nsid_e(void);\n"
    assert protos(L, text) == {"nsid_a": ("i", ""), "nsid_b": ("l", ""), "nsid_c": ("z", "i"), "nsid_d": ("c", "i"), "nsid_e": ("c", "")}
    assert L._CT["c"] is ctypes.c_char_p and L._CT["z"] is ctypes.c_size_t and L._CT["l"] is ctypes.c_long


def test_wide_integers_are_not_ints(L):
    text = "int nsid_a(int64_t n, size_t bytes, long m, int32_t k, int j, const int64_t* I, float f, double d);"
    assert protos(L, text) == {"nsid_a": ("i", "lzliipfd")}


def test_pointers_strings_and_the_stream(L):
    text = """typedef struct nsid_thing { const void* p[2]; int a, b; } nsid_thing;
    int nsid_a(const nsid_thing* things, int n, float* const* rows, const float* const* more, const char* key, long* value,
               void* stream);
    int nsid_b(void* device_buf);
    int nsid_c(const void* stream, int stream_count);"""
    assert protos(L, text) == {"nsid_a": ("i", "pippcps"), "nsid_b": ("i", "p"), "nsid_c": ("i", "pi")}


def test_typedef_block_preprocessor_lines_and_the_extern_wrapper_are_skipped(L):
    text = """#ifndef NSID_H
#define NSID_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NSID_OK 0
typedef struct nsid_wgrad_problem {
  const void* dout[2];
  int ldd, ldx;   /* a comment; with a semicolon */
} nsid_wgrad_problem;
int nsid_grouped(const nsid_wgrad_problem* problems, int n, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* NSID_H */
"""
    p, d = L.parse_header(text)
    assert p == {"nsid_grouped": ("i", "pis")} and d == {"NSID_OK": 0}


@pytest.mark.parametrize("text, named", [
    ("int nsid_a(int n, unsigned flags);", "nsid_a"),                     # unknown parameter type
    ("int nsid_a(int n, hipStream_t stream);", "nsid_a"),
    ("int nsid_a(const nsid_unknown* p);", "nsid_a"),                     # a struct the header does not define
    ("void nsid_a(int n);", "nsid_a"),                                    # unknown return type
    ("char* nsid_a(int n);", "nsid_a"),
    ("int nsid_a(int);", "nsid_a"),                                       # a parameter without a name
    ("int nsid_a(int n, void (*done)(int, void*), void* stream);", "nsid_a"),      # the comma split cannot handle it
    ("int nsid_a(int n)\nint nsid_b(int m);", "nsid_a"),                  # a lost semicolon
    ("int nsid_a(int n);\nint nsid_a(int n);", "nsid_a"),                 # declared twice
    ("int nsid_a(int n);\nstatic inline int nsid_b(int m) { return m; }", "nsid_b"),
    ("int nsid_a(int n);\n#define NSID_CALL(x) nsid_b(x)\n", "NSID_CALL"),
])
def test_what_the_parser_does_not_understand_raises_and_names_it(L, text, named):
    with pytest.raises(ImportError, match=named):
        L.parse_header(text)


def test_define_forms(L):
    text = """#ifndef NSID_H
#define NSID_H
#define NSID_OK 0
#define NSID_EINVAL (-1)   /* unsupported shape */
#define NSID_ROW_TILE 128 /* rows per tile */
  #  define   NSID_SPACED   ( +7 )
#define NSID_NEG -3
#define OTHER_PREFIX 1.5
#endif"""
    assert L.parse_header(text)[1] == {"NSID_OK": 0, "NSID_EINVAL": -1, "NSID_ROW_TILE": 128, "NSID_SPACED": 7, "NSID_NEG": -3}
    for bad in ("#define NSID_EPS 1e-5", "#define NSID_NAME \"x\"", "#define NSID_SUM (1 + 2)", "#define NSID_FLAG", "#define NSID_HALF 0.5"):
        with pytest.raises(ImportError, match=bad.split()[1]):
            L.parse_header(bad + "\n")


def test_missing_header_names_the_path(L, monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "nsid.h")
    monkeypatch.setattr(L, "HEADER_PATH", missing)
    with pytest.raises(ImportError, match="nsid.h"):
        L.load_header()


# ---- the real header

def test_every_prototype_is_bound_as_the_header_declares_it(L):
    """argtypes and restype on the loaded library, for every prototype of include/nsid.h, from the C types spelled out here"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "nsid.h")).read(), flags=re.S)
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "long": ctypes.c_long, "int64_t": ctypes.c_long, "size_t": ctypes.c_size_t,
              "float": ctypes.c_float, "double": ctypes.c_double}
    seen = 0
    for ret, name, params in re.findall(r"\b(int|long|size_t|const char\*) (nsid_\w+)\(([^)]*)\);", text):
        want = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            ctype = " ".join(p.split()).rsplit(" ", 1)[0]
            want.append(ctypes.c_char_p if ctype == "const char*" else ctypes.c_void_p if "*" in ctype else scalar[ctype])
        fn = getattr(L.lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}[ret], name
        assert L.SIGNATURES[name] == L.PROTOTYPES[name][1] and len(L.SIGNATURES[name]) == len(want)
        assert (L.SIGNATURES[name][-1:] == "s") == params.rstrip().endswith("void* stream") and "s" not in L.SIGNATURES[name][:-1]
        seen += 1
    assert seen == len(L.PROTOTYPES) == len(L.EXPORTS) >= 134
    assert set("".join(L.SIGNATURES.values())) <= set("pilzfdsc")


def test_defines_of_the_real_header(L):
    from neuralsampleid_amd import ops
    D = L.DEFINES
    assert "NSID_H" not in D and D["NSID_OK"] == 0 and D["NSID_EINVAL"] == -1 and D["NSID_ELAUNCH"] == -2
    assert D["NSID_DECLINED"] == 1 and set(L._ERR) == {-1, -2, 1}        # call() names a decline nobody expected, like an error
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY, ops.ACT_ELU) == (0, 1, 2, 3) and ops.ROW_TILE == 128
    assert (ops.F32, ops.BF16, ops.GEMM_FP32, ops.GEMM_BF16) == (0, 1, 0, 1)
    # the limits the kernels are compiled with, at the values they had as literals on both sides
    assert (ops.SEARCH_MAX_K, ops.VOTE_MAX_CAND, ops.VOTE_MAX_TOP) == (64, 4096, 32)
    assert (ops.CLF_C, ops.CLF_KP, ops.CLF_MAX_N, ops.CLF_MAX_N_EVAL, ops.CLF_QCHUNK, ops.CLF_PW, ops.CLF_HID, ops.CLF_H) == \
        (512, 1024, 32, 128, 64, 512, 128, 4)
    assert (ops.CLF_MINE_MAX_ROWS, ops.CLF_MINE_MAX_D, ops.BL_MAX, ops.BL_ROWS_MAX) == (8192, 512, 2048, 4096)
    assert (ops.AUG_N_FFT, ops.AUG_HOP, ops.AUG_BINS, ops.AUG_FX_MAX_SECTIONS, ops.AUG_FX_MAX_FRAMES) == (2048, 512, 1025, 64, 256)
    assert (ops.RESAMPLE_MAX_C, ops.RESAMPLE_LDS_BYTES, ops.DsPrep.MAX_LAYERS) == (8, 65536, 8)
    from neuralsampleid_amd import frontend, packs
    from neuralsampleid_amd.modules import transformations
    assert (packs.LOGMEL_RUN, packs.CQT_TILE, packs.TABLE_COLS, frontend.CQT_GROUP, frontend.CQT_RC) == (8, 32, 4, 8, 256)
    assert (transformations.AUG_ZEROS, transformations.AUG_PRECISION) == (64, 512)


def test_moved_limits_hold_at_the_entries(L):
    """For every moved limit that an entry checks itself and that has a launch-free way past the argument check (zero rows, pairs or
    tiles: NSID_OK with nothing launched): accepted at the limit, NSID_EINVAL at limit + 1, on a machine without a GPU. The entries
    whose only way past the check is a launch (the baseline losses, nsid_aug_biquad / _frames, nsid_resample_sinc, nsid_ds_prepack)
    keep their GPU tests."""
    from neuralsampleid_amd import ops
    lib, N = L.lib, None
    L.launch_counters(reset=True)
    K, TOP, CAND = ops.SEARCH_MAX_K, ops.VOTE_MAX_TOP, ops.VOTE_MAX_CAND
    for k, rc in ((K, 0), (K + 1, -1)):
        assert lib.nsid_flat_l2_topk(N, 128, 0, N, 128, 0, N, N, 128, k, N, N, N, 0, N) == rc, k
        assert lib.nsid_seq_scores(N, 128, N, 128, 0, 128, N, k, N, N, 0, N, 0, N) == rc, k
        assert lib.nsid_song_vote(N, k, N, 1, N, N, 0, N, 0, 0, N, 1, N, N, N, N) == rc, k
        assert lib.nsid_song_vote_clf(N, k, N, N, N, N, N, 0, N, 0, 0, N, 0.5, 1, N, N, N, N) == rc, k
    for top, rc in ((TOP, 0), (TOP + 1, -1)):
        assert lib.nsid_song_vote(N, 1, N, 1, N, N, 0, N, 0, 0, N, top, N, N, N, N) == rc, top
        assert lib.nsid_song_vote_clf(N, 1, N, N, N, N, N, 0, N, 0, 0, N, 0.5, top, N, N, N, N) == rc, top
    for lds, rc in ((CAND, 0), (CAND + 1, -1)):
        assert lib.nsid_song_vote(N, 1, N, lds, N, N, 0, N, 0, 0, N, 1, N, N, N, N) == rc, lds
    for n, rc in ((ops.CLF_MAX_N, 0), (ops.CLF_MAX_N + 1, -1)):
        assert lib.nsid_clf_node_rows(N, 0, 512, n, N, N, N) == rc, n
        assert lib.nsid_clf_pair_scores(N, 0, N, 0, n, N, N, N, 0, 0, N, N, N, 0, N) == rc, n
        assert lib.nsid_clf_pair_scores_c(N, 0, N, 0, 768, n, N, N, N, 0, 0, N, N, N, 0, N) == rc, n
        assert lib.nsid_clf_attn_fwd(N, 1, N, 1, n, N, N, 0, N, N, N, N) == rc, n
        assert lib.nsid_clf_attn_fwd_c(N, 1, N, 1, 640, n, N, N, 0, N, N, N, N) == rc, n
        assert lib.nsid_clf_attn_bwd(N, N, N, 1, N, 1, n, N, N, 0, N, N, N) == rc, n
        assert lib.nsid_clf_attn_bwd_c(N, N, N, 1, N, 1, 1024, n, N, N, 0, N, N, N) == rc, n
        assert lib.nsid_clf_seg_reduce(N, N, N, N, N, N, 0, n, 0, 0, N, N, N) == rc, n
        assert lib.nsid_clf_seg_reduce_c(N, N, N, N, N, N, 0, 512, n, 0, 0, N, N, N) == rc, n
    for n, rc in ((ops.CLF_MAX_N_EVAL, 0), (ops.CLF_MAX_N_EVAL + 1, -1)):
        assert lib.nsid_clf_node_rows_n(N, 0, 512, n, N, N, N) == rc, n
        assert lib.nsid_clf_pair_scores_n(N, 0, N, 0, 1024, n, N, N, N, 0, 0, N, N, N, 0, N) == rc, n
    rows, d = ops.CLF_MINE_MAX_ROWS, ops.CLF_MINE_MAX_D
    assert lib.nsid_clf_mine_hard_negatives(N, 0, N, rows, d, 1, N, N) == 0
    assert lib.nsid_clf_mine_hard_negatives(N, 0, N, rows + 1, d, 1, N, N) == -1
    assert lib.nsid_clf_mine_hard_negatives(N, 0, N, rows, d + 4, 1, N, N) == -1
    assert sum(L.launch_counters().values()) == 0
