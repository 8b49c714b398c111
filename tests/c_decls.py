"""The C text of a boundary that ctypes crosses, read back: the functions a header declares or a source defines under `extern "C"`, what
ctypes type each declaration stands for, and where a table name -> (restype, argtypes) disagrees with them (tests/test_abi.py holds
conflict_rez_amd/engine.py PROTOTYPES to include/confrez_hip.h with it, and the tables of the test-only bindings to their sources).
What it cannot see: two parameters of one type in swapped order.  Not a test module."""
import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "long": C.c_long, "double": C.c_double}
POINTEES = set(SCALARS) | {"void", "char", "int64_t", "uint8_t"}  # what a c_void_p may point to, besides the caller's structs
_FUNCTION = re.compile(r"^([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)$")


def _closing_brace(text, i):
    """The index after the `}` that closes the `{` at text[i]."""
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return j + 1
    raise ValueError("unbalanced braces")


def declarations(text):
    """{name: (return type, [parameter declarations])} of the functions of a C text, in its order: prototypes (ending in `;`) outside
    every block but `extern "C"`, and definitions (ending in `{`) directly inside an `extern "C"` block.  `static` functions are not
    exported and are left out; comments (the in-line shape comments of parameters among them) and preprocessor lines are dropped first."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    out, start, i, in_c = {}, 0, 0, 0
    while i < len(text):
        ch = text[i]
        i += 1
        if ch not in ";{}":
            continue
        stmt = " ".join(text[start : i - 1].split())
        if ch == "{" and re.fullmatch(r'extern\s*"C"', stmt):
            in_c += 1
        elif ch == "}":
            in_c = max(in_c - 1, 0)
        else:
            m = _FUNCTION.match(stmt)
            if m and m.group(1).split()[0] not in ("static", "typedef") and (ch == ";" or in_c):
                ret, name, params = " ".join(m.group(1).replace("*", " * ").split()), m.group(2), " ".join(m.group(3).split())
                if name in out:
                    raise ValueError(f"{name} is declared twice")
                out[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
            if ch == "{":
                i = _closing_brace(text, i - 1)  # a body, a struct, a namespace: nothing inside is a declaration
        start = i
    return out


def expected_ctypes(decl, structs=None, returns=False):
    """The ctypes type of one parameter declaration (`const double *x0`, `long counts[6]`, `int B`) or, with `returns`, of a return type
    (no name in it).  structs: {C name: its ctypes mirror, or None for a type that only ever crosses as a pointer}.  A pointer to a
    mirrored struct -> (POINTER(mirror), c_void_p), either is right (arrays of structs are passed raw); every other answer is one type.
    A base type that is neither in SCALARS, POINTEES nor structs raises: an unknown type is not a pass."""
    structs = structs or {}
    m = re.fullmatch(r"(.*?)((?:\[\w*\])*)", decl.strip())
    words = [w for w in m.group(1).replace("*", " * ").split() if w not in ("const", "struct")]
    stars = words.count("*") + bool(m.group(2))
    words = [w for w in words if w != "*"]
    if not returns and len(words) > 1:
        words = words[:-1]  # the parameter's name
    if len(words) != 1 or not (words[0] in POINTEES or words[0] in structs):
        raise ValueError(f"cannot map the C declaration `{decl}`: unknown base type {' '.join(words)!r}")
    base = words[0]
    if stars == 0:
        if base == "void" and returns:
            return None
        if base not in SCALARS:
            raise ValueError(f"cannot map the C declaration `{decl}`: {base} by value")
        return SCALARS[base]
    if stars == 1 and base == "char" and returns:
        return C.c_char_p
    if stars == 2 and base in structs and structs[base] is None:
        return C.POINTER(C.c_void_p)  # an opaque handle handed out
    if stars == 1 and structs.get(base) is not None:
        return (C.POINTER(structs[base]), C.c_void_p)
    if stars != 1:
        raise ValueError(f"cannot map the C declaration `{decl}`: {stars} levels of pointer to {base}")
    return C.c_void_p


def _agrees(got, want):
    return any(got is w for w in want) if isinstance(want, tuple) else got is want


def mismatches(prototypes, decls, structs=None):
    """Where the table `prototypes`, name -> (restype, argtypes), disagrees with `decls` (of `declarations`): a function without a row,
    a row without a function, a return type, a parameter count, a parameter's type; each as a line that names the function (and the
    parameter).  Scalars must be the very type expected_ctypes names: c_int is not taken for int32_t where the two differ."""
    out = [f"{name}: declared, but the table has no row" for name in decls if name not in prototypes]
    out += [f"{name}: a row of the table, but not declared" for name in prototypes if name not in decls]
    for name, (ret, params) in decls.items():
        if name not in prototypes:
            continue
        restype, argtypes = prototypes[name]
        if not _agrees(restype, expected_ctypes(ret, structs, returns=True)):
            out.append(f"{name}: returns `{ret}`, the table says {restype}")
        if len(argtypes) != len(params):
            out.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} in the table")
            continue
        for k, (p, t) in enumerate(zip(params, argtypes)):
            want = expected_ctypes(p, structs)
            if not _agrees(t, want):
                out.append(f"{name}: parameter {k} `{p}` is {want}, the table says {t}")
    return out
