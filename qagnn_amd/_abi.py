"""The C ABI of libqagnn_hip.so, read from the public headers (include/*.h): prototypes, structs and integer constants as ctypes.

The headers are the one statement of the ABI; _lib.py declares nothing by hand.  This is no C parser: it reads the subset of C99 the
headers are written in and REFUSES (ValueError naming the header and the text) whatever it does not recognise, because a declaration
skipped here would reach ctypes undeclared -- a device pointer passed as a 32-bit int.  No torch, no GPU, no library load.

Type rule:  int / int32_t, int64_t, uint32_t, uint64_t, uint8_t, float, double -> the ctypes type of that width;  qagnn_stream_t ->
c_void_p;  a one-level pointer to one of the ABI's own structs -> POINTER(struct);  every other pointer, whatever its depth or
constness -> c_void_p;  `const char*` as a return type -> c_char_p;  `(void)` -> [];  an array field `T name[QAGNN_X]` -> ctype * value.
"""
import ctypes as C
import functools
import glob
import os
import re

INCLUDE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include'))
SCALARS = {'int': C.c_int32, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
           'uint8_t': C.c_uint8, 'float': C.c_float, 'double': C.c_double, 'qagnn_stream_t': C.c_void_p}
_INT = re.compile(r'\(?\s*(\d+|0[xX][0-9a-fA-F]+)\s*(?:<<\s*(\d+)\s*)?\)?$')
_DECLARATOR = re.compile(r'((?:\s*\*|\s*\bconst\b)*)\s*([A-Za-z_]\w*)?\s*(?:\[\s*(\w+)\s*\])?\s*$')  # `* const* name[SIZE]`: stars, name, array size
_BASE = re.compile(r'\s*(?:const\s+)*([A-Za-z_]\w*)\b(.*)$', re.S)
_KEYWORD = re.compile(r'\b(union|struct|enum)\b')
_PROTOTYPE = re.compile(r'(.+?)\b(qagnn_[a-z0-9_]+)\s*\((.*)\)$', re.S)


class Header:
    """One header: prototypes [(name, restype, [argtypes])] in declaration order, structs {name: ctypes.Structure subclass} and defines
    {QAGNN_* name: its text} -- its own; what it includes is in `env` (the same three, merged, for resolving types and array sizes)."""

    def __init__(self, where):
        self.where, self.prototypes, self.structs, self.defines, self.env = where, [], {}, {}, None

    @property
    def names(self):
        return [p[0] for p in self.prototypes]

    def define(self, name):
        """the integer value of `#define name ...` of this header or one it includes; ValueError if its text is no integer"""
        text = self.defines[name] if name in self.defines else self.env.defines[name]
        m = _INT.match(text)
        if not m:
            raise ValueError(f'{self.where}: #define {name} {text!r} is no integer constant')
        return int(m.group(1), 0) << int(m.group(2) or 0)

    def integers(self):
        """{name: value} of this header's own defines that are integers (an include guard is none)"""
        return {n: self.define(n) for n, t in self.defines.items() if _INT.match(t)}


def _refuse(h, why, text):
    raise ValueError(f'{h.where}: {why}: {" ".join(text.split())!r}')


def _declarator(h, base, decl, text, named):
    """`base` (type name, const dropped) and one declarator (`* const* p`, `p[QAGNN_X]`) -> (name or None, ctypes type)"""
    m = _DECLARATOR.match(decl)
    if not m or (named and not m.group(2)):
        _refuse(h, 'not a declaration this parser reads', text)
    depth, name, size = m.group(1).count('*'), m.group(2), m.group(3)
    struct = h.structs.get(base) or h.env.structs.get(base)
    if depth == 0 and struct:
        _refuse(h, f'struct {base} passed or held by value', text)
    if not (struct or base in SCALARS or (depth and base in ('void', 'char'))):
        _refuse(h, f'unknown type name {base!r}', text)
    ctype = SCALARS[base] if depth == 0 else C.POINTER(struct) if depth == 1 and struct else C.c_void_p
    if size is not None:
        if not named:
            _refuse(h, 'array parameter', text)
        if not (size.isdigit() or size in h.defines or size in h.env.defines):
            _refuse(h, f'array size {size!r} is no constant defined above', text)
        ctype = ctype * (int(size) if size.isdigit() else h.define(size))
    return name, ctype


def _declaration(h, text, named):
    """`const float *a, *b` -> [(name, ctype), ...]; named: a struct field (several declarators, arrays), else a parameter or return type"""
    if '(' in text:
        _refuse(h, 'function pointer', text)
    if ':' in text:
        _refuse(h, 'bit-field', text)
    if _KEYWORD.search(text):
        _refuse(h, 'union, nested struct or enum', text)
    first, *rest = text.split(',')
    m = _BASE.match(first)
    if not m or (rest and not named):
        _refuse(h, 'not a declaration this parser reads', text)
    return [_declarator(h, m.group(1), d, text, named) for d in [m.group(2)] + rest]


def _struct(h, name, body):
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields += _declaration(h, decl, True)
    if '{' in body or '}' in body or not fields or len({n for n, _ in fields}) != len(fields):
        _refuse(h, 'struct body this parser does not read', body)
    return type(name, (C.Structure,), {'_fields_': fields, '__doc__': f'struct {name} of include/{os.path.basename(h.where)} (generated: field order is the ABI)'})


def _prototype(h, text):
    m = _PROTOTYPE.match(text)
    if not m:
        _refuse(h, 'neither a struct typedef nor a prototype', text)
    ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
    if '...' in params:
        _refuse(h, 'variadic parameter list', text)
    if '(' in params or ')' in params:
        _refuse(h, 'function pointer', text)
    if ''.join(ret.split()) == 'constchar*':
        restype = C.c_char_p
    elif ret == 'void':
        restype = None
    else:
        restype = _declaration(h, ret, False)[0][1]
    argtypes = [] if params == 'void' else [_declaration(h, p, False)[0][1] for p in params.split(',')]
    return name, restype, argtypes


def parse(text, where='<text>', env=None):
    """The declarations of one header's text -> Header.  env: the merged Header of what it includes (struct types, array sizes)."""
    h = Header(where)
    h.env = env or Header(where)
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*', ' ', text, flags=re.S | re.M)
    for line in re.findall(r'^[ \t]*#[^\n]*', text, flags=re.M):
        if line.rstrip().endswith('\\'):
            _refuse(h, 'continued preprocessor line', line)
        m = re.match(r'[ \t]*#[ \t]*define[ \t]+(QAGNN_\w+)(\(?)(.*)$', line)
        if m:
            name, value = m.group(1), (m.group(2) + m.group(3)).strip()
            if m.group(2) and not _INT.match(value):
                _refuse(h, 'function-like macro', line)
            if h.defines.setdefault(name, value) != value:
                _refuse(h, f'{name} defined twice with different values', line)
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', text, flags=re.M)
    # what is left is a sequence of `...;` at brace depth 0: typedef void* qagnn_stream_t | typedef struct X { ... } X | a prototype
    for m in re.finditer(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;|([^;{}]+);|(\S)', text, flags=re.S):
        if m.group(5):
            _refuse(h, 'text this parser does not read', text[m.start():m.start() + 80])
        if m.group(1):
            if m.group(1) != m.group(3) or m.group(1) in h.structs or m.group(1) in h.env.structs:
                _refuse(h, 'struct typedef under another name, or defined twice', m.group(0))
            h.structs[m.group(1)] = _struct(h, m.group(1), m.group(2))
        elif m.group(4).split() == ['typedef', 'void*', 'qagnn_stream_t']:
            continue
        else:
            h.prototypes.append(_prototype(h, m.group(4).strip()))
    if len(set(h.names)) != len(h.names):
        _refuse(h, 'a function declared twice', ' '.join(n for n in h.names if h.names.count(n) > 1))
    for name in re.findall(r'\b(qagnn_[a-z0-9_]+)\s*\(', text):
        if name not in h.names:
            _refuse(h, 'a call-like name that was not read as a prototype', name)
    return h


def _merged(hs, where):
    env = Header(where)
    for x in hs:
        for part in (x.env, x):
            env.structs.update(part.structs)
            env.defines.update(part.defines)
    return env


@functools.lru_cache(maxsize=None)
def header(path):
    """parse(one header file), the headers it includes with "..." first (each file is parsed once per process)"""
    with open(path) as f:
        text = f.read()
    incs = [header(os.path.join(os.path.dirname(path), i)) for i in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, re.M)]
    return parse(text, path, _merged(incs, path))


def headers():
    """{file name: Header} of every include/*.h, sorted by name"""
    return {os.path.basename(p): header(p) for p in sorted(glob.glob(os.path.join(INCLUDE, '*.h')))}
