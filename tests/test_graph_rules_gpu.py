"""GPU tests of the graph rules of the fused engine forms, on exact data (the method of test_exact_gpu.py: grid data, the float64
convolution and lp_testing.exact_epilogue give the bits of every tensor in advance).

A wrong "nobody else reads it" answer of the library raises no error: it leaves a tensor that some op reads and no kernel wrote.
NaN poison alone does not show that (a stale tensor of the previous forward of the same input is even the right value; a ReLU consumer
no longer turns NaN into 0 -- DESIGN 4.1.5 -- but a NaN behind it only says that SOMETHING upstream was unwritten), so every tensor of the arena is filled with a marked NaN pattern before the forward and EVERY tensor of
the graph is compared with its expected bits afterwards -- the one a fused form would have kept on chip included.

  * every changed graph of lp_testing's tables (the ones test_graph_rules_cpu.py shows to be refused) runs with the tuner on, the
    production path, from a frame of the engine's dtype;
  * every base graph runs with its form forced on: the carried tensors keep the marker (the fused kernel really ran), every other
    tensor is exact -- the two readers of the fused kernel's own output, one through a source and one through a residual, included;
  * whole models: with every form the library accepts switched on, every tensor some op reads is either fully written or lives
    entirely inside one fused kernel, and the prediction equals, bit for bit, the one with all forms off.
One line per graph and form is appended to graph_rules.log in the folder of the test logs (lp_testing.log_dir)."""
import os

import pytest
import torch

import lp_testing as X
import test_hip_model as M
from test_graph_rules_cpu import assert_refusals_change_nothing, carriers
from test_hip_kernels import _fill

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DT = [pytest.param(F16, id='f16'), pytest.param(BF16, id='bf16')]
DT_ID = {F16: 'f16', BF16: 'bf16'}
B = 2
FRAME = {'stem': (64, 96), 'pw': (40 << 3, 56 << 3), 'bifusion': (6 << 4, 14 << 4)}      # 1x1 + s2: maps of 40 x 56; BiFusion: 12 x 28 over 6 x 14
CASES = [pytest.param(form, change, id='%s-%s' % (form, change)) for form, (_, changes) in X.RULE_GRAPHS.items() for change in changes]
LOG_NAME = 'graph_rules.log'
_REF = {}


def _log(line):
    with open(os.path.join(X.log_dir(), LOG_NAME), 'a') as f:
        f.write(line + '\n')


@pytest.fixture(autouse=True)
def _production_switches(monkeypatch):
    for name in ('LP_NO_MFMA16', 'LP_S2P16', 'LP_TUNE_CFG128', 'LP_TUNE_NBUF', 'LP_NO_STEM_S2D', 'LP_SINGLE_LANE', 'LP_LANES', 'LP_AUTOTUNE',
                 'LP_NO_PLANAR', 'LP_NO_FUSED_STEM', 'LP_NO_FUSED_PW', 'LP_NO_FUSED_BF'):
        monkeypatch.delenv(name, raising=False)


def build(form, change, dtype):
    """The graph on the device with grid data; inputs and expected bits come from the cache (computed once, never modified)."""
    from yolov6.hip import runtime
    eng = runtime.Engine(dtype, 'cuda:0', mfma16=None)
    g = X.RULE_GRAPHS[form][0](eng, change, X.grid_rule_data(dtype))
    eng.finish()
    key = (form, change, dtype)
    if key not in _REF:
        vals = X.rule_graph_inputs(g, dtype, B, *FRAME[form])
        X.assert_grid_exact(list(vals.values()), torch.zeros(1, 1, 1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), dtype)
        want = X.rule_graph_expected(g, vals, dtype)
        for t, w in want.items():
            assert float((w != 0).float().mean()) >= 0.25, 'tensor %d of %s is mostly zero: it would not tell a stale value' % (t, key)
        _REF[key] = (vals, {t: w.cuda() for t, w in want.items()})
    vals, want = _REF[key]
    x = vals[g.t['input']].to(dtype).cuda()
    assert x.data_ptr() % 16 == 0                                         # frame_direct holds
    return eng, g, vals, want, x


def mark_and_fill(eng, g, vals):
    """The marked NaN pattern in every 16-bit element of the arena, then the graph's source tensors (no padding channels)."""
    eng.arena.view(torch.int16).fill_(X.RULE_MARK)
    for name in g.sources:
        _fill(eng, g.t[name], vals[g.t[name]])


def marked(eng, tid):
    """(some, all) stored elements of tensor ``tid`` still hold the marker."""
    m = X.engine_tensor_span(eng, tid)[2].view(torch.int16) == X.RULE_MARK
    return bool(m.any()), bool(m.all())


def check(eng, want, what, skip=()):
    bad = sum(X.bit_mismatch_count(eng.tensor_view(t), w) for t, w in want.items() if t not in skip)
    if int(bad):
        for t, w in want.items():
            if t not in skip:
                X.assert_bits(eng.tensor_view(t), w, '%s, tensor %d' % (what, t))


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('form,change', CASES)
def test_changed_graph_writes_every_tensor(form, change, dtype):
    """A graph the form must refuse, on the production path (the tuner decides): every tensor has its exact bits."""
    eng, g, vals, want, x = build(form, change, dtype)
    shape = (B,) + FRAME[form]
    assert eng.autotune
    eng.bind(*shape)
    mark_and_fill(eng, g, vals)
    eng.forward(x)                                                        # binds, tunes every op in place, runs
    assert shape in eng.tuned
    assert eng.variant(g.form_op)[0] != g.form and all(c != g.form_op for c in carriers(eng)), 'the tuner chose a form the graph rules out'
    tag = '%s %s %s' % (form, change, DT_ID[dtype])
    for run in ('tuned', 'after a refused request'):
        mark_and_fill(eng, g, vals)
        eng.forward(x)
        check(eng, want, '%s, %s' % (tag, run))
        if run == 'tuned':
            with pytest.raises(RuntimeError, match='-4'):
                eng.set_variant(g.form_op, g.form, 3)
            assert all(c != g.form_op for c in carriers(eng))
    _log('%s refused B=%d %dx%d planar=%s: %d tensors exact' % (tag, B, shape[1], shape[2], carriers(eng)[0] == 1, len(want)))


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('form', ['stem', 'planar', 'pw', 'bifusion'])
def test_base_graph_runs_the_form(form, dtype):
    """The base graph with its form forced on: the carried tensors keep the marker, everything else -- the two readers of the fused
    kernel's output included -- is exact.  Then the requests that must be refused, with the arena bound: nothing changes, the
    prepared tile included, and the form still runs."""
    planar = form == 'planar'
    gform = 'stem' if planar else form
    eng, g, vals, want, x = build(gform, None, dtype)
    shape = (B,) + FRAME[gform]
    eng.bind(*shape)
    if planar:
        eng.set_variant(1, X.PIPE_P, 3)
        kept, ops = [], [0]
        assert carriers(eng) == [1] + [-1] * (len(g.nodes) - 1)
    else:
        eng.set_variant(g.form_op, g.form, 3)
        kept, ops = [g.t[n] for n in g.carried_tensors], g.carried_ops
        assert carriers(eng) == [g.form_op if i in ops else -1 for i in range(len(g.nodes))]
    assert not eng.autotune
    if gform == 'stem':                              # the space-to-depth input, which the host never declared
        kept = kept + eng.op_io(0)[2]
    assert {'t1', 't2'} <= set(g.t) and g.nodes[g.op['t2']]['res'] == g.t[g.nodes[g.form_op]['name']]
    tag = '%s base %s' % (form, DT_ID[dtype])
    for run in ('forced', 'after refused requests'):
        mark_and_fill(eng, g, vals)
        eng.forward(x)
        check(eng, want, '%s, %s' % (tag, run), skip=kept)
        for t in kept:
            assert marked(eng, t) == (True, True), '%s, %s: carried tensor %d was written' % (tag, run, t)
        if run == 'forced' and not planar:
            assert_refusals_change_nothing(eng, g, tiles=True)
            if gform == 'stem':                      # (that walk switches the planar stem on as well: the fused stem still carries both ops)
                assert carriers(eng)[:3] == [2, 2, -1]
    _log('%s accepted, ran B=%d %dx%d: %d tensors exact, %d carried' % (tag, B, shape[1], shape[2], len(want) - len(set(kept) & set(want)), len(kept)))


# ---- whole models ---------------------------------------------------------------------------------------------------------------------
FORMS = (X.PIPE_P, X.FUSED_STEM2, X.FUSED_PW_S2, X.FUSED_BIFUSION)
ALL4 = {X.PIPE_P, X.FUSED_STEM2, X.FUSED_PW_S2, X.FUSED_BIFUSION}
# (id, forms the library must accept somewhere in the model -- DESIGN 3.1e-g, 3.1j: the stem forms want at most 32 stem channels (yolov6m
# has 48: planar only), the 1x1 + stride-2 and BiFusion forms a 64-channel BiFusion level (the width-1/16 models have 8-channel ones))
MODELS = [(c[0], {X.PIPE_P, X.FUSED_STEM2}) for c in M.MODEL_CASES] + [('yololps', ALL4), ('yololpn', ALL4), ('yolov6m', {X.PIPE_P})]


def _model_and_input(name):
    from conftest import load_golden
    from yolov6.utils.synth import build_synthetic
    for case, weights, arch in M.MODEL_CASES:
        if case == name:
            return M._tiny_model(arch, weights, True), load_golden(case)['x'][:B]
    x = torch.rand(B, 3, 128, 128, generator=torch.Generator().manual_seed(7))
    return build_synthetic(M.CFG(name)).eval(), x


def graph_of(eng):
    """{tensor: producing op}, {tensor: reading ops} from lp_engine_op_io."""
    prod, readers = {}, {}
    for i in range(eng.lib.lp_engine_num_ops(eng.h)):
        srcs, res, dsts = eng.op_io(i)
        for t in dsts:
            assert t not in prod, 'two ops write tensor %d' % t
            prod[t] = i
        for t in srcs + ([res] if res >= 0 else []):
            readers.setdefault(t, []).append(i)
    return prod, readers


def assert_no_unwritten_read(eng, what):
    """Every tensor some op reads has no marker element left, or its producer and all its readers are carried by one kernel (then
    NO element of it was written); every tensor that still holds the marker is of that second kind.  -> the tensors of the second kind."""
    prod, readers = graph_of(eng)
    car = carriers(eng)
    kernel = lambda op: car[op] if car[op] >= 0 else op
    inside = []
    for t in sorted(set(prod) | set(readers)):
        assert t in prod, '%s: tensor %d is read and no op writes it' % (what, t)
        some, every = marked(eng, t)
        on_chip = car[prod[t]] >= 0 and all(kernel(r) == kernel(prod[t]) for r in readers.get(t, []))
        if on_chip:
            assert every, '%s: tensor %d lives inside the kernel of op %d and was written' % (what, t, kernel(prod[t]))
            inside.append(t)
        else:
            assert not some, '%s: tensor %d (written by op %d, read by %s) still holds the marker' % (what, t, prod[t], readers.get(t))
    return inside


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('name,must', MODELS, ids=[m[0] for m in MODELS])
def test_model_reads_no_unwritten_tensor(name, must, dtype):
    from yolov6.hip import runtime
    m, x = _model_and_input(name)
    eng = runtime.Engine.from_model(m, dtype, torch.device('cuda:0'))
    eng.autotune = False
    x = x.to(dtype).cuda()
    eng.bind(x.shape[0], x.shape[2], x.shape[3])
    n = eng.lib.lp_engine_num_ops(eng.h)
    before = [eng.variant(i) for i in range(n)]
    on = []
    for i in range(n):
        for f in FORMS:
            try:
                eng.set_variant(i, f, 3)
                on.append((i, f))
            except RuntimeError:
                pass
    assert {f for _, f in on} == must, on
    assert [eng.variant(i)[0] for i, _ in on] == [f for _, f in on]
    preds = []
    passes = [('every form on', None)] + ([('planar stem alone', 2)] if (2, X.FUSED_STEM2) in on else []) + [('every form off', -1)]
    for what, off in passes:
        for i in ([off] if off is not None and off >= 0 else [i for i, _ in on] if off == -1 else []):
            eng.set_variant(i, *before[i])
        if off == -1:
            assert [eng.variant(i) for i in range(n)] == before and carriers(eng) == [-1] * n
        eng.arena.view(torch.int16).fill_(X.RULE_MARK)
        preds.append(eng.forward(x))
        inside = assert_no_unwritten_read(eng, '%s %s, %s' % (name, DT_ID[dtype], what))
        assert bool(torch.isfinite(preds[-1]).all())
        car = carriers(eng)
        assert len(inside) == sum(c >= 0 for c in car), (inside, car)       # one tensor per carried op stays on chip
        _log('model %s %s, %s: ran, forms %s, %d tensors on chip' % (name, DT_ID[dtype], what, [(i, eng.variant(i)[0]) for i, _ in on], len(inside)))
    for p in preds[:-1]:
        assert torch.equal(p, preds[-1]), 'the prediction with the forms on differs from the one with every form off'
