"""The C ABI read from include/cassnat_hip.h, the place that declares it (``EXTRA_FUNCTIONS`` / ``PROJ_FUNCTIONS`` / ``AST_NGRAM_FUNCTIONS`` /
``NAT_NGRAM_FUNCTIONS`` / ``CTC_TIMES_FUNCTIONS`` / ``SCORE_FUNCTIONS`` / ``CTC_BIAS_FUNCTIONS`` / ``AST_BIAS_FUNCTIONS`` / ``FEATS_FUNCTIONS``: the entry points of
its companions include/cassnat_hip_ctc_ngram.h, include/cassnat_hip_attention_proj.h, include/cassnat_hip_ast_ngram.h,
include/cassnat_hip_nat_ngram.h, include/cassnat_hip_ctc_times.h, include/cassnat_hip_score.h, include/cassnat_hip_ctc_bias.h,
include/cassnat_hip_ast_bias.h and include/cassnat_hip_feats.h, read the same way; ``CTC_MERGE_FUNCTIONS``: those of
include/cassnat_hip_ctc_merge.h; ``VAD_FUNCTIONS``: those of include/cassnat_hip_vad.h; ``ALIGN_FUNCTIONS`` / ``ALIGN_STRUCTS``: those of
include/cassnat_hip_align.h; ``GENMAX_FUNCTIONS`` / ``GENMAX_STRUCTS`` / ``GENMAX_CONSTANTS``: those of include/cassnat_hip_genmax.h): ``FUNCTIONS`` name -> (restype, argtypes),
``STRUCTS`` C name -> ctypes.Structure, ``CONSTANTS`` enum / #define name -> int.  It reads this project's header, not C in general:
what it does not recognise raises ``AbiError`` naming the declaration.  Standard library only (no torch, numpy, library or GPU)."""
import ctypes as C
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cassnat_hip.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_BASE = re.compile(r"(?:const\s+)?(\w+)\s*")
_DECL = re.compile(r"((?:\*\s*)*)(\w*)\s*(?:\[(\d+)\])?")


class AbiError(ValueError):
    pass


class Abi:
    def __init__(self):
        self.functions, self.structs, self.constants, self.opaque = {}, {}, {}, set()

    def ctype(self, base, stars, where):
        """``base`` behind ``stars`` asterisks: a scalar by value, c_char_p, POINTER(struct), or c_void_p for every other pointer."""
        if not stars and base in SCALARS:
            return SCALARS[base]
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and base in self.structs:
            return C.POINTER(self.structs[base])
        if stars and (base in SCALARS or base in self.structs or base in self.opaque or base in ("void", "char", "uint8_t")):
            return C.c_void_p
        raise AbiError(f"{where}: unknown type {base + '*' * stars!r}")

    def declarators(self, text, where):
        """``const T *a, b[3]`` -> [(name, ctypes type)]; an empty name is a bare type (``void`` alone gives None)."""
        text = " ".join(text.split())
        m = _BASE.match(text)
        out = []
        for part in text[m.end():].split(",") if m else ():
            d = _DECL.fullmatch(part.strip())
            if not d:
                raise AbiError(f"{where}: cannot read {text!r}")
            if m.group(1) == "void" and not d.group(1) and not d.group(2):
                out.append(("", None))
                continue
            t = self.ctype(m.group(1), d.group(1).count("*"), f"{where}: {text!r}")
            out.append((d.group(2), t * int(d.group(3)) if d.group(3) else t))
        if not out:
            raise AbiError(f"{where}: cannot read {text!r}")
        return out


def parse(text, base=None):
    """``base``: the Abi of a header this one includes; its structs and opaque types are known here, its functions are not repeated."""
    abi = Abi()
    if base is not None:
        abi.structs.update(base.structs)
        abi.opaque.update(base.opaque)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CN_\w+)[ \t]+(-?\w+)[ \t]*$", text, re.M):
        abi.constants[name] = int(value, 0)
    text = re.sub(r'^[ \t]*#[^\n]*|extern\s+"C"\s*\{', " ", text, flags=re.M)

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, eq, value = (s.strip() for s in item.partition("="))
            if not eq or not re.fullmatch(r"\w+", name):
                raise AbiError(f"enum: cannot read {item!r}")
            abi.constants[name] = int(value, 0)
        return " "

    def struct(m):
        fields = []
        for line in filter(None, (s.strip() for s in m.group(2).split(";"))):
            got = abi.declarators(line, f"struct {m.group(1)}")
            if any(not name or t is None for name, t in got):
                raise AbiError(f"struct {m.group(1)}: cannot read {line!r}")
            fields += got
        cls = "".join(p.title() for p in m.group(1).split("_"))
        abi.structs[m.group(1)] = type(cls, (C.Structure,), {"_fields_": fields, "__doc__": f"{m.group(1)} of include/cassnat_hip.h"})
        return " "

    text = re.sub(r"\benum\s*\{(.*?)\}\s*;", enum, text, flags=re.S)
    abi.opaque.update(re.findall(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", text))
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", " ", text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(cn_\w+)\s*\((.*)\)", stmt, re.S)
        if not m:
            if stmt == "}":  # (closes extern "C")
                continue
            raise AbiError(f"cannot split the declaration {' '.join(stmt.split())!r}")
        name, params = m.group(2), m.group(3).strip()
        ret = abi.declarators(m.group(1), f"{name}: return type")
        args = [] if params == "void" else [d for p in params.split(",") for d in abi.declarators(p, name)]
        if len(ret) != 1 or ret[0][0] or any(not n or t is None for n, t in args):
            raise AbiError(f"cannot split the declaration of {name}: {' '.join(stmt.split())!r}")
        abi.functions[name] = (ret[0][1], [t for _, t in args])
    return abi


with open(HEADER_PATH) as _f:
    HEADER = parse(_f.read())
FUNCTIONS, STRUCTS, CONSTANTS = HEADER.functions, HEADER.structs, HEADER.constants
# the companion header of the CTC prefix beam search with word n-gram fusion: functions only, over cassnat_hip.h's types
EXTRA_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_ctc_ngram.h")
with open(EXTRA_HEADER_PATH) as _f:
    EXTRA_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the attention kernel's projecting form (cn_op_attention_proj), likewise
PROJ_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_attention_proj.h")
with open(PROJ_HEADER_PATH) as _f:
    PROJ_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the AST beam search with word n-gram fusion, likewise
AST_NGRAM_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_ast_ngram.h")
with open(AST_NGRAM_HEADER_PATH) as _f:
    AST_NGRAM_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the CASS-NAT finish loop with word n-gram fusion, likewise
NAT_NGRAM_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_nat_ngram.h")
with open(NAT_NGRAM_HEADER_PATH) as _f:
    NAT_NGRAM_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the CTC token time stamps (forced alignment with spans and confidences), likewise
CTC_TIMES_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_ctc_times.h")
with open(CTC_TIMES_HEADER_PATH) as _f:
    CTC_TIMES_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the scorer's edit alignment, likewise
SCORE_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_score.h")
with open(SCORE_HEADER_PATH) as _f:
    SCORE_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the CTC prefix beam search with phrase biasing: its descriptor (cn_bias_desc) and entry points
CTC_BIAS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_ctc_bias.h")
with open(CTC_BIAS_HEADER_PATH) as _f:
    CTC_BIAS_HEADER = parse(_f.read(), base=HEADER)
CTC_BIAS_FUNCTIONS = CTC_BIAS_HEADER.functions
CTC_BIAS_STRUCTS = {"cn_bias_desc": CTC_BIAS_HEADER.structs["cn_bias_desc"]}
# the companion header of the AST beam search with phrase biasing: functions only, over cassnat_hip_ctc_bias.h's descriptor
AST_BIAS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_ast_bias.h")
with open(AST_BIAS_HEADER_PATH) as _f:
    AST_BIAS_FUNCTIONS = parse(_f.read(), base=CTC_BIAS_HEADER).functions
# the companion header of the feature-archive writer (matrix compression and CMVN sums; bin/make_fbank): functions only
FEATS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_feats.h")
with open(FEATS_HEADER_PATH) as _f:
    FEATS_FUNCTIONS = parse(_f.read(), base=HEADER).functions
# the companion header of the CTC prefix beam search that merges candidates by prefix: functions only, over cn_ngram_desc and cn_bias_desc
CTC_MERGE_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_ctc_merge.h")
with open(CTC_MERGE_HEADER_PATH) as _f:
    CTC_MERGE_FUNCTIONS = parse(_f.read(), base=CTC_BIAS_HEADER).functions
# the companion header of the energy voice-activity detector (frame energies and the decision; bin/make_segments): functions only
VAD_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_vad.h")
with open(VAD_HEADER_PATH) as _f:
    VAD_HEADER = parse(_f.read(), base=HEADER)
VAD_FUNCTIONS, VAD_CONSTANTS = VAD_HEADER.functions, VAD_HEADER.constants
# the companion header of the alignment and hypothesis kernels' single-kernel entries: its descriptor (cn_align_desc) and entry points
ALIGN_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_align.h")
with open(ALIGN_HEADER_PATH) as _f:
    ALIGN_HEADER = parse(_f.read(), base=HEADER)
ALIGN_FUNCTIONS = ALIGN_HEADER.functions
ALIGN_STRUCTS = {"cn_align_desc": ALIGN_HEADER.structs["cn_align_desc"]}
# the companion header of the fused generator tail: its descriptor (cn_genmax_desc), the form query, the pack query and their constants
GENMAX_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "cassnat_hip_genmax.h")
with open(GENMAX_HEADER_PATH) as _f:
    GENMAX_HEADER = parse(_f.read(), base=HEADER)
GENMAX_FUNCTIONS, GENMAX_CONSTANTS = GENMAX_HEADER.functions, GENMAX_HEADER.constants
GENMAX_STRUCTS = {"cn_genmax_desc": GENMAX_HEADER.structs["cn_genmax_desc"]}


def bind(L):
    """Set ``restype`` / ``argtypes`` of every declared function on the loaded library ``L``; a function a header declares and the
    library lacks raises AttributeError."""
    for name, (restype, argtypes) in list(FUNCTIONS.items()) + list(EXTRA_FUNCTIONS.items()) + list(PROJ_FUNCTIONS.items()) + list(AST_NGRAM_FUNCTIONS.items()) + list(NAT_NGRAM_FUNCTIONS.items()) + list(CTC_TIMES_FUNCTIONS.items()) + list(SCORE_FUNCTIONS.items()) + list(CTC_BIAS_FUNCTIONS.items()) + list(AST_BIAS_FUNCTIONS.items()) + list(FEATS_FUNCTIONS.items()) + list(CTC_MERGE_FUNCTIONS.items()) + list(VAD_FUNCTIONS.items()) + list(ALIGN_FUNCTIONS.items()) + list(GENMAX_FUNCTIONS.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L
