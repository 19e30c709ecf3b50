"""The ctypes binding is derived from include/cassnat_hip.h (cassnat_asr_public_amd/abi.py): the parser on a header written here,
the declarations it must refuse, the real header, and - with the libraries built - what hip.lib() set on every function.  No GPU."""
import ctypes as C
import re

import pytest

from cassnat_asr_public_amd import abi, hip

SYNTHETIC = r"""
/* a comment that names cn_fake(int x); and has (parentheses) */
#ifndef DEMO_H
#define DEMO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct cn_model cn_model;
enum { CN_KIND_A = 0, CN_KIND_B = 3 };   // cn_other( in a line comment
#define CN_FLAG 0x10
typedef struct cn_demo {
    const void* p;      /* pointer field; cn_fake( again */
    int32_t a, b;       /* several declarators */
    int32_t c;
    double d;           /* aligned to 8 behind three int32_t */
    float f;
    int32_t r[3];
    const uint64_t* q;
    int64_t n;
    uint64_t m /* a comment inside the declaration */;
} cn_demo;
const char* cn_name(void);
void cn_free(cn_model* m);
int32_t cn_count(const cn_demo* d);
int64_t cn_bytes(int32_t a, int64_t b);
int cn_everything(cn_model* m, cn_model** out, const cn_demo* desc, const char* name, char* buf, void* p,
                  const float* x, int32_t* y, const uint64_t* keys /* a note */, const uint8_t* mask,
                  int i, int32_t j, int64_t k, uint64_t l, float f, double g);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    h = abi.parse(SYNTHETIC)
    assert h.constants == {"CN_KIND_A": 0, "CN_KIND_B": 3, "CN_FLAG": 16}
    assert list(h.structs) == ["cn_demo"] and h.opaque == {"cn_model"}
    D = h.structs["cn_demo"]
    assert issubclass(D, C.Structure) and D.__name__ == "CnDemo"
    assert D._fields_ == [("p", C.c_void_p), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("d", C.c_double), ("f", C.c_float),
                          ("r", C.c_int32 * 3), ("q", C.c_void_p), ("n", C.c_int64), ("m", C.c_uint64)]
    assert [getattr(D, n).offset for n, _ in D._fields_] == [0, 8, 12, 16, 24, 32, 36, 48, 56, 64] and C.sizeof(D) == 72
    d = D(a=1, b=2)
    d.r[2] = 7
    assert (d.a, d.b, list(d.r)) == (1, 2, [0, 0, 7])
    assert sorted(h.functions) == ["cn_bytes", "cn_count", "cn_everything", "cn_free", "cn_name"]  # no cn_fake, no cn_other
    assert h.functions["cn_name"] == (C.c_char_p, [])
    assert h.functions["cn_free"] == (None, [C.c_void_p])
    assert h.functions["cn_count"] == (C.c_int32, [C.POINTER(D)])
    assert h.functions["cn_bytes"] == (C.c_int64, [C.c_int32, C.c_int64])
    assert h.functions["cn_everything"] == (C.c_int, [
        C.c_void_p, C.c_void_p, C.POINTER(D), C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double])


@pytest.mark.parametrize("text, names", [
    ("int cn_f(size_t n);", ("cn_f", "size_t")),                                   # unknown scalar
    ("int cn_g(int16_t* p);", ("cn_g", "int16_t*")),                               # unknown pointee: no silent c_void_p
    ("uint8_t cn_h(void);", ("cn_h", "uint8_t")),                                  # unknown return type
    ("typedef struct cn_s { int32_t a; int32_t (*fn)(int); } cn_s;", ("cn_s", "fn")),  # a field it cannot read
    ("typedef struct cn_t { unsigned int a; } cn_t;", ("cn_t", "unsigned int a")),
    ("int cn_k(int32_t a, int32_t);", ("cn_k",)),                                  # a parameter without a name
    ("int cn_m(int32_t a;", ("cn_m",)),                                            # a prototype it cannot split
    ("int cn_n(void (*cb)(int), int32_t a);", ("cn_n",)),
    ("enum { CN_A, CN_B };", ("CN_A",)),                                           # an enumerator without a value
])
def test_parser_refuses_what_it_does_not_recognise(text, names):
    with pytest.raises(abi.AbiError) as e:
        abi.parse(text)
    for name in names:
        assert name in str(e.value), (name, str(e.value))


STRUCT_SIZES = {"cn_config": 100, "cn_decode_opts": 64, "cn_ast_opts": 56, "cn_fbank_opts": 64, "cn_attn_desc": 200, "cn_ngram_desc": 160, "cn_chain_desc": 200,
                "cn_frontend_desc": 208, "cn_gemm_desc": 120, "cn_proj_x3_desc": 72}


def test_the_real_header():
    assert len(abi.FUNCTIONS) == 121
    assert {n: C.sizeof(s) for n, s in abi.STRUCTS.items()} == STRUCT_SIZES
    for cls, name in ((hip.CnConfig, "cn_config"), (hip.CnDecodeOpts, "cn_decode_opts"), (hip.CnAstOpts, "cn_ast_opts"),
                      (hip.CnFbankOpts, "cn_fbank_opts"), (hip.CnAttnDesc, "cn_attn_desc"), (hip.CnNgramDesc, "cn_ngram_desc"),
                      (hip.CnChainDesc, "cn_chain_desc"), (hip.CnFrontendDesc, "cn_frontend_desc"),
                      (hip.CnGemmDesc, "cn_gemm_desc"), (hip.CnProjX3Desc, "cn_proj_x3_desc")):
        assert cls is abi.STRUCTS[name]
    K = abi.CONSTANTS
    assert [K["CN_PRECISION_" + n] for n in ("F32", "BF16", "FP8", "BF16X3", "F16")] == [0, 1, 2, 3, 4]
    assert [K["CN_DTYPE_" + n] for n in ("F32", "I32", "U8", "F64")] == [0, 1, 2, 3]
    assert [K["CN_FP8_" + n] for n in ("CONV2", "LINEAR", "FFN")] == [1, 2, 4]
    assert [K["CN_GEMM_EPI_" + n] for n in ("RELU", "RESID", "EMBED", "SWISH")] == [1, 2, 4, 8]
    assert {"cn_op_gemm_desc", "cn_gemm_desc_size", "cn_gemm_form"} <= set(abi.FUNCTIONS)
    assert {"cn_op_proj_x3_desc", "cn_proj_x3_desc_size", "cn_proj_x3_form", "cn_ffn_x3_form"} <= set(abi.FUNCTIONS)
    assert [K["CN_FFN_X3_" + n] for n in ("PRO", "TAIL", "MIX", "SWISH")] == [1, 2, 4, 8]
    assert hip.PRECISION["fp32"] == hip.PRECISION["float32"] == 0 and hip.PRECISION["bf16x3"] == 3 and hip.PRECISION["float16"] == 4
    assert sorted(hip.DTYPES) == [0, 1, 2, 3] and hip.FP8_SCOPE_BITS == {"conv2": 1, "linear": 2, "ffn": 4}
    names = hip.declared_symbols()
    assert names == sorted(set(names)) and len(names) == 121 and all(n.startswith("cn_") for n in names)
    assert not set(names) & set(abi.STRUCTS) and "cn_model" not in names


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_every_declared_function_is_bound(flavour):
    """Parameter counts and return types are counted from the header's text here, apart from the parser's own reading."""
    L = hip.lib(flavour)
    with open(abi.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    returns = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "void": None, "const char*": C.c_char_p}
    seen = 0
    for ret, name, params in re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M):
        fn = getattr(L, name)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(fn.argtypes) == count == len(abi.FUNCTIONS[name][1]), name
        assert fn.restype is returns[ret.strip()], name
        seen += 1
    assert seen == len(abi.FUNCTIONS) == 121
