"""Reads a C header of the shape of include/diffute_hip.h into ctypes: one Structure per `typedef struct`, one
(restype, [argtypes]) per function declaration, the integer `#define`s and anonymous enums.  _cabi.py binds the library with the result,
so the header is the only place an entry of the C ABI is written down on the Python side.

Strict on purpose: a type, a declarator shape or a directive this file does not know raises HeaderError with the declaration in the
message - it never guesses `int` and never skips.  A wrong guess would load, run and hand a kernel a garbage pointer or size.

Mapping (one rule, no per-symbol exceptions): integer / floating scalars -> their ctypes scalars; `char*` -> c_char_p; every other pointer,
pointer to pointer and array parameter -> c_void_p (call sites pass byref(struct), ctypes arrays, c_void_p(addr) and None, all of which
c_void_p takes and a typed POINTER would not); a struct by value -> its Structure; a `void` result -> None."""
import ctypes
import keyword
import re


class HeaderError(RuntimeError):
    pass


_SCALARS = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
    "long long": ctypes.c_int64, "int64_t": ctypes.c_int64, "unsigned long long": ctypes.c_uint64, "uint64_t": ctypes.c_uint64,
    "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "unsigned char": ctypes.c_ubyte,
}
_POINTEE_ONLY = ("void", "char")              # complete only behind a `*` (`void` alone is also a result type)
_DIRECTIVES_IGNORED = ("include", "ifndef", "endif")


def camel(cname):
    """dmx_gemm_desc -> GemmDesc"""
    return "".join(w.capitalize() for w in cname.split("_")[1:])


def parse_int(text, what):
    """decimal, hex, either of them negative and / or in one pair of parentheses"""
    t = text.strip()
    if t.startswith("(") and t.endswith(")"):
        t = t[1:-1].strip()
    if not re.fullmatch(r"-?\s*(0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)", t):
        raise HeaderError(f"not an integer constant: `{what}`")
    return int(t.replace(" ", ""), 0)


class Header:
    def __init__(self):
        self.structs = {}        # header name -> ctypes.Structure subclass, in header order
        self.protos = {}         # symbol -> (restype, [argtypes])
        self.macros = {}         # NAME -> replacement text of `#define NAME text`, as written
        self.enums = {}          # enumerator -> int
        self._types = dict(_SCALARS)   # by-value types: the scalars, pointer typedefs, the structs
        self._pointees = set(_POINTEE_ONLY)   # names that may only stand behind a `*`: void, char, opaque handles
        self._params = {}        # parameter text -> ctypes type

    def constant(self, name):
        """value of an integer macro or an enumerator; a macro that is not a plain integer raises"""
        if name in self.enums:
            return self.enums[name]
        if name not in self.macros:
            raise HeaderError(f"no macro or enumerator `{name}` in the header")
        return parse_int(self.macros[name], f"#define {name} {self.macros[name]}")

    # ---- one declarator: `const float* x`, `int shape[4]`, `void* const* events`, `dmx_dpm_coefs coefs`, `void`
    def _declarator(self, text, decl):
        """-> (the words without cv-qualifiers: type, then the name if there is one; pointer depth; array length, "" for `[]`, None)"""
        toks = re.findall(r"\w+|\*|\[\s*\w*\s*\]", text)
        if "".join(toks) != re.sub(r"\s+", "", text) or not toks:
            raise HeaderError(f"declarator `{text.strip()}` not understood in `{decl}`")
        arr = None
        if toks[-1].startswith("["):
            arr = toks.pop()[1:-1].strip()
            if arr and not arr.isdigit():
                raise HeaderError(f"array length `{arr}` not a literal in `{decl}`")
        if any(t.startswith("[") for t in toks):
            raise HeaderError(f"multi-dimensional array `{text.strip()}` in `{decl}`")
        words = [t for t in toks if t != "*" and t not in ("const", "struct")]
        return words, toks.count("*"), arr

    def _base(self, words, decl):
        """split [type words..., name?] at the longest known type -> (type name, name or None)"""
        for k in range(len(words), 0, -1):
            t = " ".join(words[:k])
            if t in self._types or t in self._pointees:
                if len(words) - k > 1:
                    break
                return t, (words[k] if k < len(words) else None)
        raise HeaderError(f"unknown type in `{' '.join(words)}` of `{decl}`")

    def _ctype(self, base, ptr, decl):
        if ptr:
            return ctypes.c_char_p if (base == "char" and ptr == 1) else ctypes.c_void_p
        if base not in self._types:
            raise HeaderError(f"`{base}` cannot be passed or stored by value in `{decl}`")
        return self._types[base]

    # ---- statements
    def _function(self, stmt):
        m = re.fullmatch(r"(.+?)\b(\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            raise HeaderError(f"declaration not understood (function pointers and nested parentheses are not supported): `{stmt}`")
        res, name, params = m.groups()
        words, ptr, arr = self._declarator(res, stmt)
        base, extra = self._base(words, stmt)
        if extra is not None or arr is not None:
            raise HeaderError(f"result type not understood in `{stmt}`")
        restype = None if (base == "void" and not ptr) else self._ctype(base, ptr, stmt)
        args = []
        if params.strip() != "void":
            for p in params.split(","):
                if p not in self._params:              # (`dmx_stream_t stream`, `int ldx`, ... recur: parsed once)
                    words, ptr, arr = self._declarator(p, stmt)
                    base, _ = self._base(words, stmt)
                    self._params[p] = ctypes.c_void_p if arr is not None else self._ctype(base, ptr, stmt)
                args.append(self._params[p])
        if name in self.protos:
            raise HeaderError(f"`{name}` declared twice")
        self.protos[name] = (restype, args)

    def _struct(self, stmt, tag, body, name, class_names):
        if tag and tag != name:
            raise HeaderError(f"struct tag `{tag}` differs from its typedef name `{name}`")
        fields = []
        for line in body.split(";"):
            if not line.strip():
                continue
            decl = f"{name}: {' '.join(line.split())}"
            first, *more = line.split(",")
            words, ptr, arr = self._declarator(first, decl)
            base, fname = self._base(words, decl)
            for i, d in enumerate([None] + more):
                if i:                      # `int R, C`: the later declarators share the base type, not the first one's `*` or `[n]`
                    words, ptr, arr = self._declarator(d, decl)
                    fname = words[0] if len(words) == 1 else None
                if fname is None:
                    raise HeaderError(f"field without a name in `{decl}`")
                t = self._ctype(base, ptr, decl)
                if arr is not None:
                    if not arr or ptr:
                        raise HeaderError(f"array field `{fname}` not understood in `{decl}`")
                    t = t * int(arr)
                fields.append((fname + "_" if keyword.iskeyword(fname) else fname, t))
        cls = type(class_names.get(name) or camel(name), (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} (include/diffute_hip.h)"})
        self.structs[name] = self._types[name] = cls

    def _enum(self, stmt, body):
        nxt = 0
        for e in body.split(","):
            if not e.strip():
                continue
            name, eq, val = (s.strip() for s in e.partition("="))
            if not re.fullmatch(r"[A-Za-z_]\w*", name):
                raise HeaderError(f"enumerator `{e.strip()}` not understood in `{stmt}`")
            self.enums[name] = nxt = parse_int(val, f"{name} = {val} in {stmt}") if eq else nxt
            nxt += 1


def parse(text, class_names=None):
    """class_names: {header struct name: Python class name} for the names camel() does not give"""
    h = Header()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif\b", " ", text, flags=re.S)      # the extern "C" brackets
    rest = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            rest.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*(\w+)\s*(.*?)\s*", line)
        if m and m.group(1) == "define":
            d = re.fullmatch(r"(\w+)(?:\s+(.*))?", m.group(2))
            if not d:
                raise HeaderError(f"macro not understood (function-like macros are not supported): `{line.strip()}`")
            h.macros[d.group(1)] = d.group(2) or ""
        elif not m or m.group(1) not in _DIRECTIVES_IGNORED:
            raise HeaderError(f"preprocessor directive not understood: `{line.strip()}`")
    # statements: split at the `;` outside braces
    depth, start, body = 0, 0, "\n".join(rest)
    for m in re.finditer(r"[{};]", body):
        i, ch = m.start(), m.group()
        depth += (ch == "{") - (ch == "}")
        if ch != ";" or depth:
            continue
        stmt, start = " ".join(body[start:i].split()), i + 1
        if not stmt:
            continue
        m = re.fullmatch(r"typedef struct\s*(\w*)\s*\{(.*)\}\s*(\w+)", stmt)
        if m:
            h._struct(stmt, *m.groups(), class_names or {})
        elif re.fullmatch(r"typedef struct (\w+) \1", stmt):
            h._pointees.add(stmt.split()[-1])                                             # opaque handle
        elif re.fullmatch(r"typedef void\s*\*\s*\w+", stmt):
            h._types[re.findall(r"\w+", stmt)[-1]] = ctypes.c_void_p                       # dmx_stream_t
        elif re.fullmatch(r"enum\s*\{(.*)\}", stmt):
            h._enum(stmt, stmt[stmt.index("{") + 1:-1])
        elif stmt.startswith(("typedef", "enum", "struct", "union", "static", "extern")) or "{" in stmt:
            raise HeaderError(f"declaration not understood: `{stmt}`")
        else:
            h._function(stmt)
    if depth or body[start:].strip():
        raise HeaderError(f"text after the last declaration: `{' '.join(body[start:].split())[:80]}`")
    return h
