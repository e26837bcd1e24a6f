"""Exact-arithmetic GPU tests (the method of test_exact_gpu.py) of layer classes the kernel selection rules admit but no model or
parity case contains: sources whose K-chunks put a tap pair or a loop pass of the 16x16x32 kernels across two tensors, layers at the
edges of the kernels' LDS tables (lp_testing.RULE_ROWS, whose rule side test_rules_cpu.py pins on the CPU), and partial widths of the
fused stem.  Engines use the production default of the MFMA family, so the first forward runs what the rule picks.  Every case names
the kernel families that must have run it and, by that, the ones that must have refused it: a variant that silently stops taking
a layer fails here.  No refused configuration is ever launched: a refusal is the error of lp_engine_set_op_variant."""
import pytest
import torch

import lp_testing as X
import test_exact_gpu as E
from test_exact_gpu import ALL_VARIANTS, BF16, DT_ID, EPILOGUES, F16, F32
from test_rules_cpu import _production_switches, default_family          # noqa: F401 (autouse: the production switches)

pytestmark = pytest.mark.gpu

VARIANTS_OF = {}
for _cfg, _nb in ALL_VARIANTS:
    VARIANTS_OF.setdefault(E._family(_cfg), []).append((_cfg, _nb))


def layer_data(cins, cout, s, h, w, B, dtype):
    """Grid data of one 3x3 layer with the conditions on it asserted (CPU only): (xs, wt, bias, res, float64 pre-activation)."""
    xs, wt, bias, res = X.grid_inputs(cins, cout, 3, B, h, w, dtype, res_hw=(h // s, w // s))
    X.assert_grid_exact(xs, wt, bias, dtype)
    pre = torch.nn.functional.conv2d(torch.cat(xs, 1), wt, None, stride=s, padding=1) + bias.view(1, -1, 1, 1)
    E._assert_rounding_exercised(pre, dtype, (cins, cout, s, h, w))
    return xs, wt, bias, res, pre


def run_layer(tag, cins, cout, s, h, w, B, dtype, must_run, default=None):
    """The layer with the four epilogues on its default kernel, then on every variant and tile choice that takes it: exact bits,
    exactly the families of ``must_run`` took it, every variant of every other family was refused."""
    sl = 5 if s == 1 else 4                                          # frames of h << sl pixels: multiples of the coarsest stride (32)
    xs, wt, bias, res, pre = layer_data(cins, cout, s, h, w, B, dtype)
    pre, res_d = pre.cuda(), res.cuda()
    wants = [X.exact_epilogue(pre, a, dtype, res_d if r else None) for a, r in EPILOGUES]
    eng, ops, dsts = E._four_epilogue_engine(dtype, cins, cout, 3, s, sl, xs, wt, bias, res, B, h << sl, w << sl, mfma16=None)
    if default is not None:
        assert default_family(eng, ops[0]) == default
    x = E._frame(B, h << sl, w << sl)
    E._poison_lds()
    for d in dsts:
        eng.tensor_view(d).fill_(E.NAN)
    eng.forward(x)                                                   # the default variant as the rule planned it
    E._check(eng, dsts, wants, tag + ' default')
    for fam in sorted(X.CONV3_FAMILIES - set(must_run)):
        for cfg, nb in VARIANTS_OF[fam]:
            with pytest.raises(RuntimeError):
                eng.set_variant(ops[0], cfg, nb)
    ran = E._walk(eng, ops, dsts, wants, ALL_VARIANTS, x, '%s-%s' % (tag, DT_ID[dtype]), B)
    assert set(ran) == set(must_run), (sorted(ran), sorted(must_run))


# ---- K-chunks of 16 stored channels from several tensors ---------------------------------------------------------------------------
CROSS_S1 = [                                                         # (sources, cout, h, w): chunks per source
    ([16, 48], 128, 20, 20),           # 1 + 3: the first tap pair of the 16x16x32 family straddles the two tensors
    ([48, 80], 128, 13, 27),           # 3 + 5: the second pair straddles; ragged map
    ([32, 96], 72, 13, 27),            # 2 + 6: a four-chunk loop pass straddles, no pair does; partial cout tile
    ([16, 16, 16, 16], 128, 20, 20),   # every chunk from another tensor
    ([40, 8], 128, 12, 20),            # 3 + 1: both tensors end in a half-empty chunk
]
CROSS_S2 = [([48, 80], 128, 26, 54), ([16, 48], 128, 40, 40), ([40, 8], 96, 34, 22)]
_cross_id = lambda c: '%s-%d-%dx%d' % ('+'.join(map(str, c[0])), c[1], c[2], c[3])


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', CROSS_S1, ids=_cross_id)
def test_chunks_across_sources_stride1(case, dtype):
    """3x3 stride 1 over a concatenation whose chunk counts are odd or not multiples of four: the generic kernel, PIPE, PIPE16 and
    PIPE16_V all take it (the total is a multiple of four) and give the exact bits on every tile; the 16x16x32 family is the default."""
    cins, cout, h, w = case
    run_layer('cross-' + _cross_id(case), cins, cout, 1, h, w, 2, dtype, {'generic', 'PIPE', 'PIPE16', 'PIPE16_V'}, default='PIPE16')


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', CROSS_S2, ids=_cross_id)
def test_chunks_across_sources_stride2(case, dtype):
    """The same at stride 2: the generic kernel and S2P16 (five K-steps per chunk, any chunk count)."""
    cins, cout, h, w = case
    run_layer('cross-s2-' + _cross_id(case), cins, cout, 2, h, w, 2, dtype, {'generic', 'S2P16'}, default='generic')


# ---- the rows of the rule table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('row', X.RULE_ROWS, ids=[r[0] for r in X.RULE_ROWS])
def test_rule_edge_layers(row, dtype):
    """lp_testing.RULE_ROWS on small maps (10 x 10 at stride 1, 20 x 20 at stride 2; the 68-chunk layers 6 x 6 and 12 x 12), B = 1:
    the families the table names run the layer bit-exactly, all others refuse it -- for the 1088-channel layers every pipelined
    variant, so they stay on the generic kernel.  fp32 engines run the generic kernel only."""
    name, cins, cout, stride, pipelined, default = row
    n = (6 if sum(cins) > 1024 else 10) * stride
    half = dtype != F32
    run_layer('edge-' + name, cins, cout, stride, n, n, 1, dtype, {'generic'} | (pipelined if half else set()), default=default if half else 'generic')


# ---- partial widths of the fused stem -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('c1,c2', [(8, 24), (24, 40), (24, 64)])
def test_fused_stem_partial_widths(c1, c2, dtype):
    """LP_VARIANT_FUSED_STEM2 with a stem narrower than its K-chunks and a second layer narrower than its cout tiles (the rule admits
    stems up to 32 channels and 32- or 64-row packings of the second layer; the other tests run 16 / 32 -> 32 / 64 only): the three
    separate ops first, then, where the form takes the op, its exact bits on every tile with the stem's tensor left untouched."""
    from yolov6.hip import abi
    B, H, W = 2, 64, 96
    frame, w1, b1, w2, b2, y1, pre2 = E.fused_data('stem', c1, c2, H, W, dtype, B)
    want1, want2 = y1.float().to(dtype).cuda(), X.exact_epilogue(pre2, 'relu', dtype).cuda()
    eng = E._engine(dtype, None)
    eng.autotune = False
    a = eng.conv([eng.input_id], w1, b1, 3, 2, abi.LP_ACT_RELU, 0)
    d = eng.conv([a], w2, b2, 3, 2, abi.LP_ACT_RELU, 1)
    eng.finish()
    x = frame.to(dtype).cuda()
    eng.forward(x)
    E._check(eng, [a, d], [want1, want2], 'fused stem %d-%d: separate ops' % (c1, c2))
    tag = 'fused_stem-%d-%d-%dx%d-%s' % (c1, c2, H, W, DT_ID[dtype])
    ran = E._walk(eng, [2], [d], [want2], [(abi.LP_VARIANT_FUSED_STEM2, 3)], x, tag, B, fused_nan=[a])
    E._log('fused_stem %s taken=%s' % (tag, bool(ran.get('fused_stem'))))
    if (c1, c2) == (24, 64):
        assert ran.get('fused_stem'), 'the fused stem did not take the op'
    if ran.get('fused_stem'):
        assert torch.isnan(eng.tensor_view(a).float()).all()         # the stem's output stayed on chip: the fused kernel ran
