"""CPU test of the graph rules of the four fused engine forms (only_reader in lp_engine_finalize, stem_planar_possible,
stem2_fused_possible, pw_fused_possible, bifusion_fused_possible in the library's host code): each form skips writing a tensor, or
skips an op, because a scan of the frozen graph says that nobody else needs it.  The builders of lp_testing (stem_rule_graph,
pw_rule_graph, bifusion_rule_graph) give per form one base graph that must be accepted and, per entry of its table of changes, a
graph that differs from the base in that one thing and must be refused; a refused request must leave the engine as it was.  Engines
on the CPU with zero weights: without a bound arena lp_engine_set_op_variant only applies the rule.  The same graphs run on the GPU,
on exact data, in test_graph_rules_gpu.py."""
import pytest
import torch

import lp_testing as X

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT = [pytest.param(F16, id='f16'), pytest.param(BF16, id='bf16')]
CASES = [pytest.param(form, change, id='%s-%s' % (form, change)) for form, (_, changes) in X.RULE_GRAPHS.items() for change in changes]
PIPE_D, PIPE16_D, STREAM64 = 32, 39, 16


@pytest.fixture(autouse=True)
def _production_switches(monkeypatch):
    for name in ('LP_NO_MFMA16', 'LP_S2P16', 'LP_TUNE_CFG128', 'LP_TUNE_NBUF', 'LP_NO_STEM_S2D', 'LP_SINGLE_LANE', 'LP_LANES'):
        monkeypatch.delenv(name, raising=False)                           # read when an engine is created / finalized


def build(form, change, dtype, device='cpu'):
    from yolov6.hip import runtime
    eng = runtime.Engine(dtype, device, mfma16=None)
    g = X.RULE_GRAPHS[form][0](eng, change)
    eng.finish()
    return eng, g


def carriers(eng, direct=1):
    return [eng.lib.lp_engine_op_carrier(eng.h, i, direct) for i in range(eng.lib.lp_engine_num_ops(eng.h))]


def assert_accepts(eng, g):
    """The form switches on, and lp_engine_op_carrier names its op for every carried op and -1 elsewhere."""
    n = eng.lib.lp_engine_num_ops(eng.h)
    assert carriers(eng) == [-1] * n
    eng.set_variant(g.form_op, g.form, 3)
    assert eng.variant(g.form_op) == (g.form, 3)
    assert carriers(eng) == [g.form_op if i in g.carried_ops else -1 for i in range(n)]
    if g.form == X.FUSED_STEM2:                      # the stem forms apply to a frame of the engine's dtype only
        assert carriers(eng, 0) == [-1] * n


def assert_op_io_is_the_graph(eng, g, rewritten):
    """lp_engine_op_io against what the builder recorded; with the space-to-depth rewrite the input op writes, and the stem reads,
    a tensor the host never declared."""
    assert eng.lib.lp_engine_num_ops(eng.h) == len(g.nodes)
    for n in g.nodes:
        srcs, res, dsts = eng.op_io(n['op'])
        want_src, want_dst = list(n.get('srcs', [])), list(n['dsts'])
        if rewritten and n['op'] == 0:
            assert len(dsts) == 1 and dsts[0] not in g.chan, dsts
            s2d = dsts[0]
            continue
        if rewritten and n['op'] == 1:
            want_src = [s2d]
        assert (srcs, res, dsts) == (want_src, -1 if n.get('res') is None else n['res'], want_dst), n


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('form', list(X.RULE_GRAPHS))
def test_base_graph_is_accepted(form, dtype):
    eng, g = build(form, None, dtype)
    assert_op_io_is_the_graph(eng, g, rewritten=form == 'stem')
    assert_accepts(eng, g)
    if form == 'stem':                               # the planar stem alone carries the input op; under the fused stem nothing changes
        n = len(g.nodes)
        eng.set_variant(1, X.PIPE_P, 3)
        assert eng.variant(1) == (X.PIPE_P, 3) and carriers(eng) == [2, 2] + [-1] * (n - 2)
        eng2, g2 = build(form, None, dtype)
        eng2.set_variant(1, X.PIPE_P, 3)
        assert carriers(eng2) == [1] + [-1] * (n - 1) and carriers(eng2, 0) == [-1] * n


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('form,change', CASES)
def test_changed_graph_is_refused(form, change, dtype):
    """Every negative is one step away from an accepted graph: the same builder with the change switched off is accepted."""
    assert_accepts(*build(form, None, dtype))
    eng, g = build(form, change, dtype)
    n = len(g.nodes)
    rewritten = form == 'stem' and change != 'input_second_reader'
    assert_op_io_is_the_graph(eng, g, rewritten)
    before = X.engine_state(eng)
    with pytest.raises(RuntimeError, match='-4'):                         # LP_ERR_UNSUPPORTED
        eng.set_variant(g.form_op, g.form, 3)
    assert carriers(eng) == [-1] * n and carriers(eng, 0) == [-1] * n
    assert X.engine_state(eng) == before
    if form == 'stem':
        if X.STEM_CHANGES[change]:                   # the stem still has its only reader of the input: the planar form applies
            eng.set_variant(1, X.PIPE_P, 3)
            assert carriers(eng) == [1] + [-1] * (n - 1)
            with pytest.raises(RuntimeError, match='-4'):
                eng.set_variant(g.form_op, g.form, 3)                     # ... and the fused form is refused beside it as well
            assert carriers(eng) == [1] + [-1] * (n - 1) and eng.variant(1) == (X.PIPE_P, 3)
        else:
            with pytest.raises(RuntimeError, match='-4'):
                eng.set_variant(1, X.PIPE_P, 3)
            assert X.engine_state(eng) == before
    if change == 'input_second_reader':              # no space-to-depth rewrite: op 0 still writes the input tensor, both readers read it
        inp = g.t['input']
        assert eng.op_io(0) == ([], -1, [inp])
        assert eng.op_io(1)[0] == [inp] and eng.op_io(g.op['x1'])[0] == [inp]


@pytest.mark.parametrize('form', list(X.RULE_GRAPHS))
def test_fp32_engine_refuses_the_form(form):
    eng, g = build(form, None, F32)
    before = X.engine_state(eng)
    with pytest.raises(RuntimeError, match='-4'):
        eng.set_variant(g.form_op, g.form, 3)
    if form == 'stem':
        with pytest.raises(RuntimeError, match='-4'):
            eng.set_variant(1, X.PIPE_P, 3)
    assert X.engine_state(eng) == before and carriers(eng) == [-1] * len(g.nodes)


def refused_requests(g):
    """Requests lp_engine_set_op_variant must refuse on the base graphs, as (op, cfg, nbuf): the other fused forms, the form itself
    with a ring depth of 2, pipelined variants that do not fit the op (a stride-2 or 1x1 layer; the stem's single K-chunk), a tile the
    library does not have, the streaming kernel on a 3x3 layer."""
    forms = (X.PIPE_P, X.FUSED_STEM2, X.FUSED_PW_S2, X.FUSED_BIFUSION)
    out = [(g.form_op, f, 3) for f in forms if f != g.form] + [(g.form_op, g.form, 2), (g.form_op, PIPE_D, 3), (g.form_op, PIPE16_D, 3),
                                                               (g.form_op, 99, 1)]
    if g.form == X.FUSED_STEM2:
        out += [(1, f, 3) for f in forms if f != X.PIPE_P] + [(1, X.PIPE_P, 2), (1, PIPE16_D, 3), (1, 99, 1), (1, STREAM64, 2),
                                                              (g.form_op, STREAM64, 2)]
    return out


def assert_refusals_change_nothing(eng, g, tiles):
    eng.set_variant(g.form_op, g.form, 3)
    if g.form == X.FUSED_STEM2:
        eng.set_variant(1, X.PIPE_P, 3)
    before = X.engine_state(eng, tiles)
    assert before[g.form_op][0] == (g.form, 3)
    for op, cfg, nbuf in refused_requests(g):
        with pytest.raises(RuntimeError, match='-4'):
            eng.set_variant(op, cfg, nbuf)
        assert X.engine_state(eng, tiles) == before, 'the refused request (op %d, variant %d, nbuf %d) changed the engine' % (op, cfg, nbuf)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('form', list(X.RULE_GRAPHS))
def test_refused_request_changes_nothing(form, dtype):
    """With the form on, a request that is refused leaves every op's variant and every op's carrier as they were."""
    eng, g = build(form, None, dtype)
    assert_refusals_change_nothing(eng, g, tiles=False)
