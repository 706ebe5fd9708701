"""The ctypes binding against the public headers it is generated from (qagnn_amd/_abi.py reads include/*.h; _lib.py declares nothing by
hand).  All `-m "not gpu"`: the struct layouts and constants against the host C compiler, written-out prototypes that between them use
every row of the type rule, one refusal per construct the parser does not read, and the loaded library with every prototype declared.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import helpers
from qagnn_amd import _abi, _lib

H = _abi.headers()
MAIN = H['qagnn_hip.h']
i32, i64, u32, u64, u8, f32, f64, vp = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_uint8, C.c_float, C.c_double, C.c_void_p
P = C.POINTER
S = MAIN.structs

# (restype, [argtypes]) copied by hand from the headers' text
KNOWN = {
    'qagnn_last_error': (C.c_char_p, []),
    'qagnn_dual_launches': (i64, []),
    'qagnn_radam_step_scaled_f32': (i32, [i32, vp, vp, vp, vp, vp, f64, f64, f64, f64, f64, f64, i32, vp, vp]),
    'qagnn_grad_norm_f32': (i32, [i32, vp, vp, f64, vp, vp, vp]),
    'qagnn_gather_multi_sum_f32': (i32, [P(S['qagnn_gather_tabs']), vp, vp, i32, i32, vp, vp]),
    'qagnn_pool_attn_fwd_f32': (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, f32, f32, u64, vp, vp, vp, vp]),
    'qagnn_head_post_bwd_f32': (i32, [vp] * 7 + [i64, vp] + [i32] * 7 + [f32, f32, u64, u64] + [vp] * 6 + [i32, vp]),
    'qagnn_timing_read': (i32, [vp, vp]),
    'qagnn_gemm_nn_dual_f32': (i32, [P(S['qagnn_gemm_nn_args']), vp, i32, P(S['qagnn_gemm_nn_args']), vp, i32, vp, i64, vp]),
    'qagnn_stack_bwd_deferred_f32': (i32, [P(S['qagnn_hop_args']), i32, vp, i64, vp]),
}


def _all_prototypes():
    return {name: (restype, argtypes) for h in H.values() for name, restype, argtypes in h.prototypes}


def test_headers_parse_to_the_exports_structs_and_constants_of_the_binding():
    assert list(H) == sorted(f for f in os.listdir(os.path.join(helpers.ROOT, 'include')) if f.endswith('.h')) and len(H) == 8
    counts = {f: len(h.prototypes) for f, h in H.items()}
    assert counts == {'qagnn_hip.h': 63, 'qagnn_hip_defer.h': 3, 'qagnn_hip_dual.h': 6, 'qagnn_hip_explain.h': 3, 'qagnn_hip_infer.h': 5,
                      'qagnn_hip_loss.h': 3, 'qagnn_hip_rows.h': 6, 'qagnn_hip_tn.h': 4}
    assert len(_all_prototypes()) == 93  # no name twice across the headers
    assert {n: len(c._fields_) for n, c in S.items()} == {'qagnn_graph': 29, 'qagnn_store': 9, 'qagnn_gemm_nn_args': 28, 'qagnn_pack_desc': 8,
                                                          'qagnn_gather_tabs': 2, 'qagnn_hop_args': 68}
    assert all(not h.structs for f, h in H.items() if f != 'qagnn_hip.h')
    for name, cls in S.items():
        assert getattr(_lib, name) is cls and issubclass(cls, C.Structure)
    assert _lib.EXPORTS == MAIN.names and _lib.EXPORTS_DUAL == H['qagnn_hip_dual.h'].names and _lib.EXPORTS_ROWS == H['qagnn_hip_rows.h'].names
    assert (_lib.CLS_SLICES, _lib.GATHER_MAX, _lib.HOP_AMAX_WORDS, _lib.ROWS_CHUNK, _lib.ROWS_MAX_N, _lib.ROWS_MAX_TABLE, _lib.DEFER_MAX_HOPS,
            _lib.TRACE_MAX_N, _lib.LOSS_THREADS) == (4, 160, 16, 64, 1 << 20, 1 << 26, 16, 1024, 256)
    assert _lib.LOSS_KINDS == {'cross_entropy': 0, 'margin_rank': 1}
    assert (_lib.HOP_AM_X, _lib.HOP_AM_S, _lib.HOP_AM_AGGR, _lib.HOP_AM_H1, _lib.HOP_AM_Y, _lib.HOP_AM_DOUT, _lib.HOP_AM_DH1,
            _lib.HOP_AM_DKMQ) == tuple(range(8))
    with open(_abi.__file__) as f:
        assert not re.search(r'^\s*(import|from)\s+(torch|\.)', f.read(), re.M), '_abi.py imports neither torch nor the package'


def test_struct_layouts_and_constants_equal_the_host_compiler():
    """A C99 program that includes all eight headers prints sizeof of every struct, offsetof of every generated field and the value of every
    parsed constant: a dropped or misnamed field does not compile, a mistyped one shifts an offset."""
    cc = shutil.which('cc') or (os.environ.get('CC') and shutil.which(os.environ['CC']))
    if not cc:
        pytest.skip('no host C compiler (cc or $CC)')
    lines, expect = [], []
    for name, cls in S.items():
        lines.append(f'printf("sizeof {name} %zu\\n", sizeof({name}));')
        expect.append(f'sizeof {name} {C.sizeof(cls)}')
        for field, _ in cls._fields_:
            lines.append(f'printf("offsetof {name} {field} %zu\\n", offsetof({name}, {field}));')
            expect.append(f'offsetof {name} {field} {getattr(cls, field).offset}')
    defines = {n: v for h in H.values() for n, v in h.integers().items()}
    assert len(defines) == 26 and defines['QAGNN_ROWS_MAX_TABLE'] == 1 << 26 and defines['QAGNN_EHIP'] == 3
    for n, v in defines.items():
        lines.append(f'printf("define {n} %lld\\n", (long long)({n}));')
        expect.append(f'define {n} {v}')
    src = ('#include <stddef.h>\n#include <stdio.h>\n' + ''.join(f'#include "{f}"\n' for f in H) +
           'int main(void) {\n  ' + '\n  '.join(lines) + '\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, 'layout.c'), 'w') as f:
            f.write(src)
        exe = os.path.join(tmp, 'layout')
        subprocess.run([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(helpers.ROOT, 'include'), '-o', exe, os.path.join(tmp, 'layout.c')],
                       check=True, capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 6 + sum(len(c._fields_) for c in S.values()) + 26
    assert out == expect, [(a, b) for a, b in zip(out, expect) if a != b]
    # the figures the C compiler gave when the binding was still written by hand
    assert [C.sizeof(S[n]) for n in ('qagnn_graph', 'qagnn_store', 'qagnn_gemm_nn_args', 'qagnn_pack_desc', 'qagnn_gather_tabs', 'qagnn_hop_args')] \
        == [200, 64, 200, 40, 1288, 480]
    hop, nn = S['qagnn_hop_args'], S['qagnn_gemm_nn_args']
    assert (hop.seed.offset, hop.ws_elems.offset, hop.s_amax.offset, nn.a_rows.offset) == (240, 424, 472, 184)


@pytest.mark.parametrize('name', list(KNOWN))
def test_prototypes_equal_their_written_out_answers(name):
    assert _all_prototypes()[name] == KNOWN[name]


def test_struct_fields_equal_their_written_out_answers():
    assert S['qagnn_store']._fields_ == [('blobs', vp), ('blob_off', vp), ('concept_ids', vp), ('node_type', vp), ('node_scores', vp),
                                         ('adj_len', vp), ('S', i32), ('n', i32), ('W', i64)]
    assert S['qagnn_gather_tabs']._fields_ == [('p', vp * 160), ('n', i32)]
    hop = dict(S['qagnn_hop_args']._fields_)
    assert [n for n, _ in S['qagnn_hop_args']._fields_[:7]] == ['g', 'N', 'DP', 'SP', 'HP', 'T', 'qscale']
    assert (hop['g'], hop['qscale'], hop['ntype'], hop['seed'], hop['ws_elems'], hop['side_stream'], hop['amax']) \
        == (P(S['qagnn_graph']), f32, vp, u64, i64, vp, vp)


def test_every_row_of_the_type_rule_on_a_synthetic_header():
    h = _abi.parse('''
        /* a comment with qagnn_not_a_function( in it */
        #define QAGNN_T_LEN (1 << 3)   // and a line comment
        #define QAGNN_T_HEX 0x10
        #define QAGNN_T_TEXT "abc"
        typedef void* qagnn_stream_t;
        typedef struct qagnn_t_a { int32_t x, y; const float *a, *b; uint8_t m[QAGNN_T_LEN]; double* const* pp[2]; } qagnn_t_a;
        typedef struct qagnn_t_b { const qagnn_t_a* a; qagnn_t_a** aa; qagnn_stream_t s; uint32_t u; } qagnn_t_b;
        const char* qagnn_t_name(void);
        int qagnn_t_f(int a, int32_t b, int64_t c, uint32_t d, uint64_t e, uint8_t f, float g, double h, qagnn_stream_t s,
                      const qagnn_t_b* one, qagnn_t_b* const* two, float* const* p, const uint32_t* q, void* r, const char* t);
        int64_t qagnn_t_g(void);
        void qagnn_t_v(const void*);
    ''', 'synthetic.h')
    assert h.integers() == {'QAGNN_T_LEN': 8, 'QAGNN_T_HEX': 16} and h.define('QAGNN_T_LEN') == 8
    a, b = h.structs['qagnn_t_a'], h.structs['qagnn_t_b']
    assert a._fields_ == [('x', i32), ('y', i32), ('a', vp), ('b', vp), ('m', u8 * 8), ('pp', vp * 2)]
    assert b._fields_ == [('a', P(a)), ('aa', vp), ('s', vp), ('u', u32)]
    assert h.prototypes == [('qagnn_t_name', C.c_char_p, []),
                            ('qagnn_t_f', i32, [i32, i32, i64, u32, u64, u8, f32, f64, vp, P(b), vp, vp, vp, vp, vp]),
                            ('qagnn_t_g', i64, []), ('qagnn_t_v', None, [vp])]


REFUSED = {
    'unknown type name': 'int qagnn_x(size_t n);',
    'unknown type behind a pointer': 'int qagnn_x(const hipStream_t* s);',
    'two-word type': 'int qagnn_x(unsigned int n);',
    'struct passed by value': 'typedef struct qagnn_s { int32_t a; } qagnn_s;\nint qagnn_x(qagnn_s s);',
    'struct held by value': 'typedef struct qagnn_s { int32_t a; } qagnn_s;\ntypedef struct qagnn_t { qagnn_s s; } qagnn_t;',
    'function-pointer parameter': 'int qagnn_x(void (*cb)(int), int32_t n);',
    'function-pointer field': 'typedef struct qagnn_s { int (*cb)(void); } qagnn_s;',
    'variadic list': 'int qagnn_x(const char* fmt, ...);',
    'union': 'typedef union qagnn_u { int32_t a; float b; } qagnn_u;',
    'union field': 'typedef struct qagnn_s { union { int32_t a; float b; } u; } qagnn_s;',
    'bit-field': 'typedef struct qagnn_s { uint32_t a : 3; uint32_t b : 29; } qagnn_s;',
    'array size that is no constant': 'typedef struct qagnn_s { float p[QAGNN_NOWHERE]; } qagnn_s;',
    'two functions in one declaration': 'int qagnn_x(void), qagnn_y(void);',
    'a definition': 'static inline int qagnn_x(void) { return 0; }',
    'function-like macro': '#define QAGNN_CALL(x) qagnn_x(x)\nint qagnn_x(int32_t x);',
    'macro use that looks like a call': 'int qagnn_x(int32_t x);\nQAGNN_API(qagnn_y(3));',
    'void by value': 'int qagnn_x(void v);',
}


@pytest.mark.parametrize('what', list(REFUSED))
def test_parser_refuses_what_it_does_not_read(what):
    with pytest.raises(ValueError, match=r'refused\.h'):
        _abi.parse('typedef void* qagnn_stream_t;\n' + REFUSED[what], 'refused.h')


def test_non_integer_define_raises_when_asked_for():
    h = _abi.parse('#define QAGNN_SCALE 0.5f\n#define QAGNN_NAME "x"\n#define QAGNN_GUARD_H\n#define QAGNN_N 7\n', 'refused.h')
    assert h.integers() == {'QAGNN_N': 7}
    for name in ('QAGNN_SCALE', 'QAGNN_NAME', 'QAGNN_GUARD_H'):
        with pytest.raises(ValueError, match=r'refused\.h.*' + name):
            h.define(name)
    with pytest.raises(KeyError):
        h.define('QAGNN_ABSENT')


def test_loaded_library_has_every_prototype_declared():
    from qagnn_amd.build import build
    build(verbose=False)
    lib = _lib.load_library()
    protos = _all_prototypes()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == argtypes, name
    # a second reading of the headers, comments and all: whatever looks like a function there is declared too
    for f in H:
        with open(os.path.join(helpers.ROOT, 'include', f)) as fh:
            for name in set(re.findall(r'\b(qagnn_[a-z0-9_]+)\s*\(', fh.read())):
                assert name in protos, f'{name} in {f}'
    touched = [n for n in vars(lib) if n.startswith('qagnn_')]
    assert len(touched) == 93 and all(getattr(lib, n).argtypes is not None for n in touched)
    assert lib.qagnn_abi_version() == _lib.ABI_VERSION and lib.qagnn_dual_launches() == 0


def test_library_without_a_declared_symbol_is_an_oserror_that_names_it():
    import _ctypes
    other = _ctypes.__file__  # some shared object that is not ours
    with pytest.raises(OSError, match=r'qagnn_last_error.*include/qagnn_hip\.h.*rebuild'):
        _lib.load_library(other)
    with pytest.raises(OSError, match='not found'):
        _lib.load_library(os.path.join(helpers.ROOT, 'no_such_library.so'))
