"""The ctypes prototype of every function include/mp2g.h declares, read from the header itself: the one place the Python host
learns an argument's or a return's width. Every parameter of the ABI is a pointer (or array) or one of five scalar types; anything
else is refused here, so a new type in the header cannot go untyped."""
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t}
_DECL = re.compile(r"([A-Za-z_][\w\s\*]*?)\b(mp2g_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, name, ret):
    """the ctypes type of one parameter declaration (with or without its name), or of a return type"""
    words = [w for w in decl.split() if w != "const"]
    if "*" in decl or "[" in decl:
        return ctypes.c_char_p if ret and words[0].rstrip("*") == "char" else ctypes.c_void_p
    if ret and words == ["void"]:
        return None
    if words and words[0] in SCALARS and len(words) <= (1 if ret else 2):
        return SCALARS[words[0]]
    raise TypeError(f"include/mp2g.h: {name}: no ctypes type for '{decl.strip()}'")


def prototypes(header_path):
    """{name: (restype, [argtypes])} of every mp2g_* function the header declares"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(header_path).read(), flags=re.S)  # comments, then preprocessor lines
    text = re.sub(r"^[ \t]*#[^\n]*", ";", text, flags=re.M)
    table = {}
    for ret, name, params in _DECL.findall(text):
        params = [] if params.strip() in ("", "void") else params.split(",")
        table[name] = (_ctype(ret, name, True), [_ctype(p, name, False) for p in params])
    return table
