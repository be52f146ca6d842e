"""ctypes binding of libeat_hip.so (the C ABI declared in include/eat_hip.h, include/eat_tag.h, include/eat_embed.h,
include/eat_attn.h, include/eat_detect.h, include/eat_sed.h, include/eat_event_score.h, include/eat_psds.h,
include/eat_weak_sed.h, include/eat_median_bank.h, include/eat_search.h, include/eat_search_q8.h, include/eat_match.h and include/eat_match_q8.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, an
exception is raised.  Build it with ``python -m efficientat_amd.build`` (or
``__graft_entry__.build()``).
"""
import ctypes
import os
import re

import torch  # noqa: F401  -- must be imported BEFORE libeat_hip.so is loaded: the kernels have to run on
#                torch's own HIP runtime (libamdhip64 bundled with the wheel) to share its streams.
#                Loading our library first binds it to /opt/rocm's copy, which sees no device.

_HERE = os.path.dirname(os.path.abspath(__file__))
# EAT_LIB: another build of the same library (A/B of kernel changes; must export the same symbols)
LIB_PATH = os.environ.get("EAT_LIB") or os.path.join(_HERE, "libeat_hip.so")
# the one declaration of the C ABI: the ctypes signatures below are parsed from it
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_hip.h")
# the long-recording tagger's entry points (efficientat_amd/tagger.py): same library, same conventions, their own header
TAG_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_tag.h")
# the embedding extractor's entry point (efficientat_amd/embeddings.py): likewise
EMBED_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_embed.h")
# the attention-pooling head's entry points (efficientat_amd/mn.py, mn_train.py): likewise
ATTN_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_attn.h")
# sound event detection's entry points (efficientat_amd/detection.py): likewise
DETECT_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_detect.h")
# strong-label SED training's entry points (efficientat_amd/sed.py, mn_train.FrameHead): likewise
SED_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_sed.h")
# event-based scoring's entry point (efficientat_amd/sed.py: evaluate_events): likewise
EVENT_SCORE_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_event_score.h")
# PSDS counting's entry point (efficientat_amd/sed.py: evaluate_psds): likewise
PSDS_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_psds.h")
# weak-label SED training's entry points (efficientat_amd/sed.py: WeakFrameTrainer): likewise
WEAK_SED_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_weak_sed.h")
# the width-bank median's entry point (efficientat_amd/sed.py: tune_postprocessing, detection.py): likewise
MEDIAN_BANK_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_median_bank.h")
# query-by-example search's entry points (efficientat_amd/retrieval.py): likewise
SEARCH_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_search.h")
# the 8-bit search index's entry points (efficientat_amd/retrieval.py, storage="q8"): likewise
SEARCH_Q8_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_search_q8.h")
# occurrence search's entry points (efficientat_amd/retrieval.py: EmbeddingIndex.find): likewise
MATCH_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_match.h")
# occurrence search over the 8-bit index (efficientat_amd/retrieval.py: EmbeddingIndex.find(allow_q8=True)): likewise
MATCH_Q8_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "eat_match_q8.h")


class EatHipError(RuntimeError):
    pass


# the whole type vocabulary of include/eat_hip.h; any pointer parameter and eat_stream_t are c_void_p
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}
_RESTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(eat_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, proto):
    """ctypes type of one parameter declaration ("const float* x", "long long n", "int")."""
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    for n in (2, 1):        # "long long", then one-word types; what follows the type is the parameter's name
        kind = " ".join(words[:n])
        if len(words) in (n, n + 1) and (kind in _SCALARS or kind == "eat_stream_t"):
            return _SCALARS.get(kind, ctypes.c_void_p)
    raise EatHipError(f"eat_hip.h: parameter type of '{decl.strip()}' in '{proto}' is outside int/float/double/long long/eat_stream_t/pointer")


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every `ret eat_name(params);` in the text of a C header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(" " if line.lstrip().startswith("#") else line for line in text.split("\n"))
    protos = {}
    for m in _PROTOTYPE.finditer(text):
        proto = " ".join(m.group(0).split())
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        if ret not in _RESTYPES:
            raise EatHipError(f"eat_hip.h: return type '{ret}' of '{proto}' is outside int/long long/const char*")
        params = m.group(3).strip()
        args = [] if params in ("", "void") else [_ctype(d, proto) for d in params.split(",")]
        protos[m.group(2)] = (_RESTYPES[ret], args)
    return protos


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_prototypes(_f.read())                           # every entry point the header declares
SIGNATURES = {name: args for name, (_, args) in PROTOTYPES.items()}    # name -> argtypes
with open(TAG_HEADER_PATH) as _f:
    TAG_PROTOTYPES = parse_prototypes(_f.read())                       # bound by lib() as well; not part of PROTOTYPES
with open(EMBED_HEADER_PATH) as _f:
    EMBED_PROTOTYPES = parse_prototypes(_f.read())                     # likewise
with open(ATTN_HEADER_PATH) as _f:
    ATTN_PROTOTYPES = parse_prototypes(_f.read())                      # likewise
with open(DETECT_HEADER_PATH) as _f:
    DETECT_PROTOTYPES = parse_prototypes(_f.read())                    # likewise
with open(SED_HEADER_PATH) as _f:
    SED_PROTOTYPES = parse_prototypes(_f.read())                       # likewise
with open(EVENT_SCORE_HEADER_PATH) as _f:
    EVENT_SCORE_PROTOTYPES = parse_prototypes(_f.read())               # likewise
with open(PSDS_HEADER_PATH) as _f:
    PSDS_PROTOTYPES = parse_prototypes(_f.read())                      # likewise
with open(WEAK_SED_HEADER_PATH) as _f:
    WEAK_SED_PROTOTYPES = parse_prototypes(_f.read())                  # likewise
with open(MEDIAN_BANK_HEADER_PATH) as _f:
    MEDIAN_BANK_PROTOTYPES = parse_prototypes(_f.read())               # likewise
with open(SEARCH_HEADER_PATH) as _f:
    SEARCH_PROTOTYPES = parse_prototypes(_f.read())                    # likewise
with open(SEARCH_Q8_HEADER_PATH) as _f:
    SEARCH_Q8_PROTOTYPES = parse_prototypes(_f.read())                 # likewise
with open(MATCH_HEADER_PATH) as _f:
    MATCH_PROTOTYPES = parse_prototypes(_f.read())                     # likewise
with open(MATCH_Q8_HEADER_PATH) as _f:
    MATCH_Q8_PROTOTYPES = parse_prototypes(_f.read())                  # likewise

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EatHipError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU/PyTorch fallback). "
                "Build it with `python -m efficientat_amd.build`.")
        h = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in (list(PROTOTYPES.items()) + list(TAG_PROTOTYPES.items()) + list(EMBED_PROTOTYPES.items())
                                          + list(ATTN_PROTOTYPES.items()) + list(DETECT_PROTOTYPES.items())
                                          + list(SED_PROTOTYPES.items()) + list(EVENT_SCORE_PROTOTYPES.items())
                                          + list(PSDS_PROTOTYPES.items()) + list(WEAK_SED_PROTOTYPES.items())
                                          + list(MEDIAN_BANK_PROTOTYPES.items()) + list(SEARCH_PROTOTYPES.items())
                                          + list(SEARCH_Q8_PROTOTYPES.items()) + list(MATCH_PROTOTYPES.items())
                                          + list(MATCH_Q8_PROTOTYPES.items())):
            fn = getattr(h, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = h
    return _lib


def call(name, *args):
    h = lib()
    rc = getattr(h, name)(*args)
    if rc != 0:
        raise EatHipError(f"{name} failed ({rc}): {h.eat_last_error_string().decode()}")


def call_rc(name, *args):
    """Like `call` for the entry points that answer 1 = "not applicable, nothing launched" (the caller takes another path)."""
    h = lib()
    rc = getattr(h, name)(*args)
    if rc not in (0, 1):
        raise EatHipError(f"{name} failed ({rc}): {h.eat_last_error_string().decode()}")
    return rc


def exported_symbols():
    return list(PROTOTYPES)
