"""What the C-ABI headers under include/ declare, read from their text: the prototypes and the two structs the Python binding mirrors, each
type mapped to the ctypes type the binding (clibd_amd._lib.HEADERS) must use for it.  The headers keep to a plain subset of C — one
declaration per `;`, `type name` parameters, `*` written next to the type, no function pointers — and anything outside it raises instead of
being skipped, so a prototype this reader cannot follow fails tests/test_abi.py."""
import ctypes as C
import re
from pathlib import Path

from clibd_amd._lib import GemmEpilogue

INCLUDE = Path(__file__).resolve().parents[1] / "include"
SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "int32_t": C.c_int32,
           "int64_t": C.c_int64}


def headers() -> list[Path]:
    return sorted(INCLUDE.glob("clibd_hip*.h"))


def strip_comments(text: str) -> str:
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def mentioned_symbols(path: Path) -> list[str]:
    """every `clibd_*(` outside comments: the names the headers were compared by before the prototypes were read"""
    return sorted(set(re.findall(r"\b(clibd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S))))


def ctype_of(c_type: str, returned: bool = False):
    """`const float*` -> c_void_p, `size_t` -> c_size_t, ...; an unknown type raises"""
    words = [w for w in c_type.replace("*", " * ").split() if w not in ("const", "struct")]
    if words.count("*") == 1 and words[-1] == "*" and len(words) >= 2:      # one level of pointer, to whatever (`unsigned char`, a struct)
        if returned:
            if words[:-1] != ["char"]:
                raise ValueError(f"no ctypes return type for {c_type!r}")
            return C.c_char_p
        return C.POINTER(GemmEpilogue) if words[:-1] == ["clibd_gemm_epilogue"] else C.c_void_p
    if len(words) == 1 and words[0] in SCALARS:
        return SCALARS[words[0]]
    raise ValueError(f"no ctypes type for {c_type!r}")


def _split_declarator(decl: str) -> tuple[str, str]:
    m = re.fullmatch(r"\s*(.*?[\s*])([A-Za-z_]\w*)\s*", decl, flags=re.S)
    if not m:
        raise ValueError(f"not a `type name` declaration: {decl!r}")
    return m.group(1), m.group(2)


def prototypes(path: Path) -> dict:
    """{name: (restype, [argtypes])} of every function the header declares"""
    text = "\n".join(ln for ln in strip_comments(path.read_text()).splitlines() if not ln.lstrip().startswith("#"))
    text = re.sub(r"\{[^{}]*\}", "", text.replace('extern "C" {', ""))     # struct and enum bodies
    out = {}
    for decl in text.split(";"):
        if "(" not in decl:
            continue
        m = re.fullmatch(r"\s*(.*?[\s*])(clibd_\w+)\s*\(([^()]*)\)\s*", decl, flags=re.S)
        if not m:
            raise ValueError(f"{path.name}: not a prototype this reader follows: {' '.join(decl.split())!r}")
        ret, name, args = m.groups()
        if name in out:
            raise ValueError(f"{path.name}: {name} is declared twice")
        args = [] if args.strip() in ("", "void") else [ctype_of(_split_declarator(a)[0]) for a in args.split(",")]
        out[name] = (ctype_of(ret, returned=True), args)
    return out


def struct_fields(path: Path, name: str) -> list[tuple]:
    """[(field, ctype)] of `struct name`, in the header's order; `int32_t a, b;` declares two fields"""
    m = re.search(r"\bstruct\s+" + name + r"\s*\{([^{}]*)\}", strip_comments(path.read_text()))
    if not m:
        raise ValueError(f"{path.name} declares no struct {name}")
    fields = []
    for decl in m.group(1).split(";"):
        if not decl.strip():
            continue
        first, *more = decl.split(",")
        c_type, field = _split_declarator(first)
        if more and "*" in decl:
            raise ValueError(f"{path.name}: pointer fields are declared one per line: {decl.strip()!r}")
        fields += [(f.strip(), ctype_of(c_type)) for f in [field] + more]
    return fields
