"""The contract of the natively sequenced hop between library, binding and operator layer (csrc/hop.hip, include/qagnn_hip.h, qagnn_amd/_lib.py):

  * `-m "not gpu"`: the binding's names of the amax words are the header's; the two workspace queries, which are the totals of the layouts the
    hops carve (HopFwdWs / HopBwdWs), behave like sizes over a grid of shapes (needs the built library, no device);
  * `-m gpu`: a hop whose workspace is 4 floats short of the query is refused by every entry point before anything is enqueued -- the zeroing
    of the amax words included.  ("Exactly the query suffices" is what every other hop test runs: the binding allocates exactly the query.)
"""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import helpers
from qagnn_amd import _lib
from test_head_widths import CANARY, EINVAL, _canaried_hop
from test_hip_kernels import edge_case, hip

AM_NAMES = ('X', 'S', 'AGGR', 'H1', 'Y', 'DOUT', 'DH1', 'DKMQ')


def test_the_binding_mirrors_the_amax_words_of_the_header():
    """`-m "not gpu"`.  QAGNN_HOP_AM_* and QAGNN_HOP_AMAX_WORDS read out of include/qagnn_hip.h against _lib.HOP_AM_* / HOP_AMAX_WORDS."""
    with open(os.path.join(helpers.ROOT, 'include', 'qagnn_hip.h')) as f:
        text = f.read()
    words = [int(v) for v in re.findall(r'#define QAGNN_HOP_AMAX_WORDS (\d+)', text)]
    found = re.findall(r'#define QAGNN_HOP_AM_(\w+) (\d+)', text)
    assert len(words) == 1 and sorted(n for n, _ in found) == sorted(AM_NAMES), (words, found)
    header = {n: int(v) for n, v in found}
    assert words[0] == _lib.HOP_AMAX_WORDS
    assert header == {n: getattr(_lib, f'HOP_AM_{n}') for n in AM_NAMES}
    assert len(set(header.values())) == len(AM_NAMES) and all(0 <= v < words[0] for v in header.values()), header


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='needs the built library (python -m qagnn_amd.build); no device')
def test_the_workspace_queries_behave_like_sizes():
    """`-m "not gpu"`.  Both queries over N x DP x SP x cls_part_rows with Ep = N + 7: a positive multiple of 4 floats (every region is padded
    to 16 bytes), growing with N (Ep * 4 floats of edge scratch alone grow by 4 per node), and a backward with a score half (SP > 0: one more
    weight-gradient product to size the split-K partials for) never below the one without."""
    lib = _lib.load_library()
    rows = [1, 200, 8191, 8192, 32768]
    for DP, SP, cls_rows in itertools.product([16, 64, 208, 256], [0, 16, 112], [0, 2, 640]):
        fwd = [lib.qagnn_hop_fwd_workspace_elems(N, N + 7, DP) for N in rows]
        bwd = [lib.qagnn_hop_bwd_workspace_elems(N, N + 7, DP, SP, cls_rows) for N in rows]
        bwd0 = [lib.qagnn_hop_bwd_workspace_elems(N, N + 7, DP, 0, cls_rows) for N in rows]
        what = (DP, SP, cls_rows, fwd, bwd)
        assert all(v > 0 and v % 4 == 0 for v in fwd + bwd), what
        assert all(a < b for a, b in zip(fwd, fwd[1:])) and all(a < b for a, b in zip(bwd, bwd[1:])), what
        assert all(a >= b for a, b in zip(bwd, bwd0)), what + (bwd0,)


def _without_S(h):
    """the hop with no score half: SP = 0 and none of its operands or gradients"""
    h.SP, h.S, h.Ws_t, h.Ws, h.dWs_t, h.dS = 0, None, None, None, None, None
    return h


@pytest.mark.gpu
@pytest.mark.parametrize('HP', [4, 16, 52])
@pytest.mark.parametrize('entry', ['hop_fwd', 'stack_fwd', 'hop_bwd', 'stack_bwd'])
def test_a_workspace_below_the_query_is_refused_before_anything_runs(entry, HP):
    """qagnn_{hop,stack}_{fwd,bwd}_f32 with ws_elems = the query - 4 (the buffer itself keeps its full size), with and without S: QAGNN_EINVAL
    from check_hop, and every saved buffer, gradient, workspace element and amax word keeps its canary.  The row threshold of the three-MFMA
    form is lowered to 1, so the forward entry points would zero the amax words first if the size were checked where the hop carves; the
    stacks hold a second hop with a full workspace that would run first (hop 0 of the forward, hop 1 of the backward)."""
    K = hip()
    ei, et, nt, R, T = edge_case('rand_small', 28).graph
    g, nt = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), nt.cuda()
    backward, stack = entry.endswith('bwd'), entry.startswith('stack')
    fn = getattr(K.lib, f'qagnn_{entry}_f32')
    with helpers.form_everywhere():
        for with_S in (True, False):
            short = _canaried_hop(K, g, nt, HP, backward)
            good = _canaried_hop(K, g, nt, HP, backward) if stack else None
            for h in [o[0] for o in (short, good) if o is not None]:
                if not with_S:
                    _without_S(h)
            h = short[0]
            query = (K.lib.qagnn_hop_bwd_workspace_elems(g.N, g.Ep, h.DP, h.SP, g.cls_part_rows) if backward
                     else K.lib.qagnn_hop_fwd_workspace_elems(g.N, g.Ep, h.DP))
            assert short[1][-1].numel() >= query  # (_canaried_hop sized it for its own SP: no smaller)
            h.ws_elems = query - 4
            order = [short] if not stack else ([short, good] if backward else [good, short])
            hops = (_lib.qagnn_hop_args * len(order))(*[o[0] for o in order])
            rc = fn(hops, len(order), K._stream()) if stack else fn(C.byref(hops[0]), K._stream())
            torch.cuda.synchronize()
            assert rc == EINVAL and b'too small' in K.lib.qagnn_last_error(), (rc, K.lib.qagnn_last_error().decode())
            for _h, guarded, keep in order:
                assert all(bool((t == CANARY).all()) for t in guarded), f'{entry}, S {with_S}: a refused call wrote to a buffer'
                assert bool((keep[4] == 123).all()), f'{entry}, S {with_S}: a refused call wrote to the amax words'
