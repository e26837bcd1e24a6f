"""Containment tests of the engine's kernels and of the NMS: an op writes every stored channel of its destinations (padding channels
as zero) and no other byte.

The exact tests say what the written bytes must be; here the same references are used again and the statement is about all the
OTHER bytes.  Engines are laid out so that an overrun has somewhere to land where it is seen (``Guarded``): front guard, sources,
residual, then per destination a guard, the destination, a guard -- each guard a tensor no op touches, as large as the destination it
protects (the engine places every declared tensor except a network input that the space-to-depth rewrite replaced: asserted from
lp_engine_tensor_info).  Before a forward the whole arena allocation is filled with the byte 0xA5 (finite in all three dtypes), the
sources get their grid data with ZERO padding channels, every destination is filled with NaN, padding channels included, and a
snapshot is taken (lp_testing.ByteWatch).  After it: (a) the logical channels carry the exact bits, (b) every padding channel of a
written tensor is zero, (c) no byte changed outside the stored intervals of the tensors the forward writes -- guards, sources,
residual, the slack behind every tensor, the unaligned head of the allocation, the arena's 256-byte tail and the allocation's slack.
That the checker would notice is shown on every case by shrinking its allowed set by one 16-byte granule at the front of one
destination and at the back of another: it must flag exactly the bytes of those granules that the forward changed.  No wrong kernel
is run anywhere.  Every (family, variant, tile) that was checked is appended to containment.log in the folder of the test logs."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
import test_exact_gpu as E
from test_exact_gpu import ALL_VARIANTS, BF16, DT_ID, EPILOGUES, F16, F32, GENERIC, NAN, PIPE
from test_hip_kernels import _engine, _poison_lds, _rand

pytestmark = pytest.mark.gpu

LOG_NAME = 'containment.log'
POISON = 0xA5
RECORD = {}          # kernel family -> {(TH, TW)} checked in this session ((0, 0): a family without tiles)
ALL3 = pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
HALF = pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])


def _log(line):
    with open(os.path.join(X.log_dir(), LOG_NAME), 'a') as f:
        f.write(line + '\n')


def _act_id(act):
    from yolov6.hip import abi
    return {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU}[act]


class Guarded:
    """An engine whose destinations lie between guard tensors, with the bookkeeping of the three assertions."""

    def __init__(self, dtype, mfma16=False):
        self.eng = _engine(dtype, mfma16)
        self.eng.autotune = False
        self.dtype = dtype
        self.names = {self.eng.input_id: 'network input'}
        self.dsts, self.guards = [], {}

    def tensor(self, c, sl, name):
        tid = self.eng.tensor(c, sl)
        self.names[tid] = name
        return tid

    def dest(self, c, sl):
        """guard, destination, guard: three tensors of the same (c, sl).  -> the destination's id."""
        i = len(self.dsts)
        g0 = self.tensor(c, sl, 'guard before dst%d' % i)
        d = self.tensor(c, sl, 'dst%d' % i)
        g1 = self.tensor(c, sl, 'guard after dst%d' % i)
        self.dsts.append(d)
        self.guards[d] = (g0, g1)
        return d

    def conv(self, srcs, wt, bias, k, s, act, sl_out, res=None, alpha=0.0, c2=0):
        """One conv op into guarded destinations (``c2``: channels of the second destination of a two-destination launch)."""
        from yolov6.hip.runtime import _f32
        w, b = _f32(wt), _f32(bias)
        d1 = self.dest(w.shape[0] - c2, sl_out)
        d2 = self.dest(c2, sl_out) if c2 else -1
        self.eng._add_conv(srcs, w, b, k, s, _act_id(act), d1, d2, res, alpha)
        return (d1, d2) if c2 else d1

    def bind(self, B, H, W):
        """Finalize, bind to an arena that starts 64 bytes past a 256-byte boundary (so that the allocation has an unaligned head of
        192 bytes in front of the arena proper), and assert the placement of the guards."""
        eng = self.eng
        if not eng.lib.lp_engine_weight_bytes(eng.h):
            eng.finish()
        n = max(self.names) + 1                             # the space-to-depth input, if finalize appended one
        z, i = ctypes.c_size_t(), [ctypes.c_int() for _ in range(4)]
        self.s2d = None
        if eng.lib.lp_engine_tensor_info(eng.h, n, ctypes.byref(z), *[ctypes.byref(v) for v in i]) == 0:
            self.names[n], self.s2d = 'space-to-depth input', n
        self.need = need = eng.lib.lp_engine_arena_bytes(eng.h, B, H, W)
        assert need > 0
        raw = torch.zeros(need + 256 + 64, dtype=torch.uint8, device='cuda:0')
        assert raw.data_ptr() % 256 == 0
        eng.arena = raw[64:]
        eng.bind(B, H, W)
        self.span = {t: X.engine_tensor_span(eng, t) for t in self.names}
        self.chan = {t: eng.tensor_view(t).shape[1] for t in self.names}
        # (the network input is not placed once the space-to-depth tensor has replaced it: Tensor::unused in lp_engine.hip)
        self.placed = [t for t in self.names if not (t == eng.input_id and self.s2d is not None)]
        self.regions = X.arena_regions(eng, self.names, self.placed)
        self.base = base = (eng.arena.data_ptr() + 255) // 256 * 256 - eng.arena.data_ptr()
        assert base == 192 and self.regions[0] == ('unaligned head', 0, 192) and self.regions[-1][0] == 'allocation slack'
        self.up = up = lambda o: base + (o - base + 255) // 256 * 256
        for d, (g0, g1) in self.guards.items():             # every destination has a placed guard directly before and after it
            (a0, b0, _), (a, b, _), (a1, b1, _) = self.span[g0], self.span[d], self.span[g1]
            assert b0 - a0 == b - a == b1 - a1 > 0 and up(b0) == a and up(b) == a1, (self.names[d], a0, b0, a, b, a1, b1)
        return self

    def full(self, tid):
        return self.span[tid][2]

    def prepare(self, fills, nan=()):
        """0xA5 everywhere, the sources' grid data with zero padding, NaN in every destination (and in ``nan``); snapshot."""
        eng = self.eng
        eng.arena.fill_(POISON)
        for tid, x in fills.items():
            self.full(tid).zero_()
            v = eng.tensor_view(tid)
            v.copy_(x.to(v.device, v.dtype))
        self.nan_extra = list(nan)
        self.poison()
        self.watch = X.ByteWatch(eng.arena, self.regions)

    def poison(self):
        for d in self.dsts + self.nan_extra:
            self.full(d).fill_(NAN)

    def allowed(self, written):
        return [self.span[t][:2] for t in written]

    def check(self, wants, written, what):
        """(a) exact bits of ``wants`` = [(tensor id, expected NCHW)], (b) zero padding channels of the ``written`` tensors, (c) no
        changed byte outside them: one device synchronisation, details only on a failure."""
        eng, iv = self.eng, X.INT_VIEW[self.dtype]
        zero = torch.zeros((), dtype=torch.int64, device='cuda:0')
        bits, pad_bad, neg0 = zero.clone(), zero.clone(), zero.clone()
        for d, w in wants:
            bits = bits + X.bit_mismatch_count(eng.tensor_view(d), w)
        for d in written:
            pad = self.full(d)[..., self.chan[d]:]
            if pad.numel():
                pad_bad = pad_bad + (pad != 0).sum()                   # (NaN != 0: an unwritten channel counts)
                neg0 = neg0 + ((pad == 0) & (pad.contiguous().view(iv) != 0)).sum()
        got = torch.stack([bits, pad_bad, neg0, self.watch.count(self.allowed(written))]).tolist()
        if got[0]:
            for i, (d, w) in enumerate(wants):
                X.assert_bits(eng.tensor_view(d), w, '%s, output %d' % (what, i))
        if got[1]:
            for d in written:
                pad = self.full(d)[..., self.chan[d]:].float()
                bad = int((pad != 0).sum())
                assert not bad, '%s: %d of %d padding elements of %s are not zero (%d of them NaN, i.e. never written)' % (
                    what, bad, pad.numel(), self.names[d], int(torch.isnan(pad).sum()))
        if got[2]:
            _log('negative zero in %d padding elements: %s' % (got[2], what))
        if got[3]:
            self.watch.assert_contained(self.allowed(written), what)

    def assert_sensitive(self, written, front, back, what):
        """The checker with the allowed set shrunk by the first 16 bytes of ``front`` and the last 16 of ``back`` flags exactly the
        bytes of those two granules that differ from the snapshot (both were NaN and are now written)."""
        (a0, b0), (a1, b1) = self.span[front][:2], self.span[back][:2]
        others = [iv for t, iv in zip(written, self.allowed(written)) if t not in (front, back)]
        r = self.watch.report(others + ([(a0 + 16, b1 - 16)] if front == back else [(a0 + 16, b0), (a1, b1 - 16)]))
        cur, snap = self.eng.arena.cpu().numpy(), self.watch.snap.cpu().numpy()
        removed = sorted(set(range(a0, a0 + 16)) | set(range(b1 - 16, b1)))
        expect = [o for o in removed if cur[o] != snap[o]]
        assert r['offsets'].tolist() == expect and r['count'] == len(expect), (what, r, expect)
        assert sum(o < a0 + 16 for o in expect) >= 4 and sum(o >= b1 - 16 for o in expect) >= 4, (what, expect)
        assert [reg[0] for reg in r['regions']] == [self.names[t] for t in sorted({front, back}, key=lambda t: self.span[t][0])], r


def _walk(g, ops, wants, written, variants, x, tag, B):
    """As test_exact_gpu._walk -- every variant of ``variants`` that takes the ops, tile choices 0..3 (a choice that repeats the tile
    before it is skipped), poisoned LDS in front of the pipelined kernels -- with the three containment assertions after every
    forward.  Returns {family: {(TH, TW)}} of what ran."""
    eng, ran = g.eng, {}
    for cfg, nb in variants:
        try:
            for op in ops:
                eng.set_variant(op, cfg, nb)
        except RuntimeError:
            continue                                        # the variant does not fit the layer (or the dtype)
        prev = None
        for choice in range(4):
            try:
                for op in ops:
                    eng.set_tile(op, choice)
                th, tw = eng.tile(ops[0])[1:]
            except RuntimeError:
                if choice > 0:
                    break                                   # no tiles, or no further candidate
                th = tw = 0
            if (th, tw) == prev:
                continue
            prev = (th, tw)
            if cfg >= 32:
                _poison_lds()
            g.poison()
            eng.forward(x)
            fam = E._family(cfg)
            g.check(wants, written, '%s variant %d/%d choice %d tile %dx%d' % (tag, cfg, nb, choice, th, tw))
            ran.setdefault(fam, set()).add((th, tw))
            RECORD.setdefault(fam, set()).add((th, tw))
            _log('%s:%d/%d B=%d choice=%d TH=%d TW=%d %s contained' % (fam, cfg, nb, B, choice, th, tw, tag))
    return ran


# ---- A. the conv families ------------------------------------------------------------------------------------------------------------
A_KEYS = [
    ((128,), 128, 3, 1, 20, 20),               # ragged map
    ((32,), 64, 3, 2, 64, 48),                 # stride 2
    ((64, 64), 128, 3, 1, 24, 16),             # two sources
    ((96,), 96, 3, 1, 16, 24),                 # residual case of the parity tests, cout no tile multiple
    ((5,), 5, 3, 1, 8, 8),                     # padded storage on both sides
    ((3,), 32, 3, 2, 64, 64),                  # 3-of-8 source padding
    ((64, 64, 64, 64), 64, 1, 1, 12, 20),      # four sources
    ((256,), 128, 1, 1, 20, 20),               # streaming 1x1
    ((64,), 96, 3, 1, 33, 17),                 # the smallest PIPE16_CASES shape: 561 pixels, several tiles of every 16x16x32 kernel
    ((96,), 200, 3, 2, 34, 22),                # the smallest S2P16_CASES shape: a ragged 17 x 11 output, two cout tiles
]
A_CASES = [c for c in X.exact_conv_cases() if c[1:7] in A_KEYS]
assert len(A_CASES) == len(A_KEYS), [c[0] for c in A_CASES]


def _conv_engine(dtype, cins, cout, k, s, sl, xs, wt, bias, res, B, H, W, epilogues=EPILOGUES):
    """The guarded form of test_exact_gpu._four_epilogue_engine: front guard, sources, residual, then guard / destination / guard
    per epilogue."""
    g = Guarded(dtype)
    sl_out = sl + (1 if s == 2 else 0)
    g.tensor(cins[0], sl, 'front guard')
    srcs = [g.tensor(c, sl, 'src%d' % i) for i, c in enumerate(cins)]
    res_id = g.tensor(cout, sl_out, 'residual')
    dsts = [g.conv(srcs, wt, bias, k, s, a, sl_out, res=res_id if r else None, alpha=X.RES_ALPHA if r else 0.0) for a, r in epilogues]
    g.bind(B, H, W)
    fills = dict(zip(srcs, xs))
    fills[res_id] = res
    g.prepare(fills)
    return g, list(range(1, 1 + len(dsts))), dsts


@ALL3
@pytest.mark.parametrize('case', A_CASES, ids=[c[0] for c in A_CASES])
def test_conv_families_write_only_their_destinations(case, dtype):
    """none / ReLU x without / with residual of a reduced list of the exact tests' cases: every variant that takes the layer -- generic
    A..F x ring depth, streaming 1x1, PIPE, PIPE16, PIPE16_V, S2P16 -- on every tile choice 0..3."""
    name, cins, cout, k, s, h, w, B = case
    sl = 5 if h <= 64 else 3
    H, W = h << sl, w << sl
    xs, wt, bias, res = X.grid_inputs(cins, cout, k, B, h, w, dtype, res_hw=(h // s, w // s))
    X.assert_grid_exact(xs, wt, bias, dtype)
    pre = E._conv64(case, xs, wt, k, s) + bias.cuda().view(1, -1, 1, 1)
    wants = [X.exact_epilogue(pre, a, dtype, res.cuda() if r else None) for a, r in EPILOGUES]
    g, ops, dsts = _conv_engine(dtype, cins, cout, k, s, sl, xs, wt, bias, res, B, H, W)
    written = [g.eng.input_id] + dsts
    x = E._frame(B, H, W)
    tag = '%s-%s' % (name, DT_ID[dtype])
    g.eng.forward(x)                                                 # the default variant as planned
    g.check(list(zip(dsts, wants)), written, tag + ' default')
    g.assert_sensitive(written, dsts[0], dsts[-1], tag)
    ran = _walk(g, ops, list(zip(dsts, wants)), written, ALL_VARIANTS, x, tag, B)
    assert 'generic' in ran


# ---- B. two destinations in one launch ----------------------------------------------------------------------------------------------
B_KEYS = [((96,), 64, 64, 1), ((64,), 64, 64, 3), ((16,), 8, 24, 3)]        # a 1x1 with a partial K-chunk, the head towers' 3x3, 8 + 24 in one cout tile
B_CASES = [c for c in E.PAIRS if (tuple(c[0]),) + tuple(c[1:4]) in B_KEYS]
assert len(B_CASES) == len(B_KEYS)


@ALL3
@pytest.mark.parametrize('case', B_CASES, ids=lambda c: '%s-%d+%d-k%d' % ('+'.join(map(str, c[0])), c[1], c[2], c[3]))
def test_two_destination_launch_writes_only_its_two_destinations(case, dtype):
    """lp_conv_desc.dst2 (the second destination's base pointer is shifted back by the channel split): guards around BOTH
    destinations, none and ReLU, every family that takes the op."""
    cins, c1, c2, k, h, w, B = case
    sl = 5
    xs, wt, bias, pre = E.pair_data(case, dtype)
    g = Guarded(dtype)
    g.tensor(cins[0], sl, 'front guard')
    srcs = [g.tensor(c, sl, 'src%d' % i) for i, c in enumerate(cins)]
    wants = []
    for act in ('none', 'relu'):
        d1, d2 = g.conv(srcs, wt, bias, k, 1, act, sl, c2=c2)
        y = X.exact_epilogue(pre, act, dtype)
        wants += [(d1, y[:, :c1].cuda()), (d2, y[:, c1:].cuda())]
    g.bind(B, h << sl, w << sl)
    assert g.eng.lib.lp_engine_num_ops(g.eng.h) == 3                 # input + two pair ops
    g.prepare(dict(zip(srcs, xs)))
    written = [g.eng.input_id] + g.dsts
    x = E._frame(B, h << sl, w << sl)
    tag = 'pair-%s-%d+%d-k%d-%s' % ('+'.join(map(str, cins)), c1, c2, k, DT_ID[dtype])
    g.eng.forward(x)
    g.check(wants, written, tag + ' default')
    g.assert_sensitive(written, g.dsts[1], g.dsts[0], tag)           # the front of a SECOND destination, the back of a first
    ran = _walk(g, [1, 2], wants, written, ALL_VARIANTS, x, tag, B)
    assert 'generic' in ran


# ---- C. the other ops ----------------------------------------------------------------------------------------------------------------
@ALL3
@pytest.mark.parametrize('cin,cout,h,w', [(16, 24, 6, 6), (64, 64, 10, 14)])
def test_deconv2x2_writes_only_its_destination(cin, cout, h, w, dtype):
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    B = 2
    x0, wt, bias, pre = E.deconv_data(cin, cout, h, w, dtype, B)
    want = X.exact_epilogue(pre, 'none', dtype).cuda()
    g = Guarded(dtype)
    g.tensor(cin, 5, 'front guard')
    src = g.tensor(cin, 5, 'src0')
    dst = g.dest(cout, 4)
    abi.check(g.eng.lib.lp_engine_add_deconv2x2(g.eng.h, src, dst, g.eng._ptr(_f32(wt)), g.eng._ptr(_f32(bias))))
    g.bind(B, h * 32, w * 32)
    g.prepare({src: x0})
    written = [g.eng.input_id, dst]
    x = E._frame(B, h * 32, w * 32)
    tag = 'deconv-%d-%d-%dx%d-%s' % (cin, cout, h, w, DT_ID[dtype])
    g.eng.forward(x)
    g.check([(dst, want)], written, tag + ' default')
    g.assert_sensitive(written, dst, dst, tag)
    assert 'generic' in _walk(g, [1], [(dst, want)], written, GENERIC, x, tag, B)


@ALL3
@pytest.mark.parametrize('c,h,w', [(8, 4, 3), (64, 13, 7), (32, 2, 1), (12, 5, 4)])
def test_pool_chain_writes_only_its_three_destinations(c, h, w, dtype):
    """Three destinations with guards between them; 12 channels: stored as 16, the pools of the four zero padding channels are zero."""
    from yolov6.hip import abi
    B = 2
    g = Guarded(dtype)
    g.tensor(c, 5, 'front guard')
    src = g.tensor(c, 5, 'src0')
    ids = [g.dest(c, 5) for _ in range(3)]
    abi.check(g.eng.lib.lp_engine_add_pool5_chain(g.eng.h, src, *ids))
    g.bind(B, h * 32, w * 32)
    x = _rand((B, c, h, w), 6).to(dtype).float()
    g.prepare({src: x})
    g.eng.forward(E._frame(B, h * 32, w * 32))
    wants, y = [], x
    for t in ids:
        y = F.max_pool2d(y, 5, 1, 2)
        wants.append((t, y.to(dtype).cuda()))                        # max is exact in every dtype
    written = [g.eng.input_id] + ids
    tag = 'pool-%d-%dx%d-%s' % (c, h, w, DT_ID[dtype])
    g.check(wants, written, tag)
    g.assert_sensitive(written, ids[1], ids[0], tag)
    RECORD.setdefault('pool', set()).add((0, 0))
    _log('pool B=%d %s contained' % (B, tag))


@ALL3
@pytest.mark.parametrize('xdtype', [F32, F16], ids=['x32', 'x16'])
def test_network_input_writes_all_eight_stored_channels_and_nothing_else(dtype, xdtype):
    """The input op alone: [B,3,H,W] -> the 8-channel tensor.  That tensor is the first of the arena (the unaligned head of the
    allocation lies in front of it, a guard tensor behind it); channels 3..7 come out zero over a NaN pre-fill; x is not modified."""
    g = Guarded(dtype)
    g.tensor(3, 0, 'guard after the network input')
    B, H, W = 2, 64, 96
    g.bind(B, H, W)
    inp = g.eng.input_id
    assert g.span[inp][0] == g.base and g.regions[1][0] == 'network input'     # directly behind the unaligned head
    g.dsts = [inp]
    g.prepare({})
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(7)).to(xdtype).cuda()
    x0 = x.clone()
    g.eng.forward(x)
    tag = 'input-%s-%s' % (DT_ID[dtype], DT_ID[xdtype])
    g.check([(inp, x0.float().to(dtype))], [inp], tag)
    g.assert_sensitive([inp], inp, inp, tag)
    assert torch.equal(x, x0)
    RECORD.setdefault('input', set()).add((0, 0))
    _log('input B=%d %s contained' % (B, tag))


def _s2d(x):
    """The space-to-depth form of an NCHW frame: channel c*4 + py*2 + px of pixel (Y, X) holds x[c][2Y+py][2X+px] (lp_aux.hip)."""
    B, C, H, W = x.shape
    return x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, C * 4, H // 2, W // 2)


@ALL3
@pytest.mark.parametrize('cout', [8, 24])
def test_stem_and_space_to_depth_input(cout, dtype):
    """Input op in its second form + the stem on a 64 x 96 frame (the widths of test_fused_stem_partial_widths): the 16-channel
    space-to-depth tensor (the arena's last tensor: a guard in front of it, the arena's tail behind it) gets 12 channels of the frame
    and four of zero over a NaN pre-fill, from an fp32 frame and from one of the engine's dtype; the frame is not modified.  Then the
    planar stem, which reads the frame itself: on every tile the stem's destination is written and the space-to-depth tensor keeps
    its pre-fill."""
    from yolov6.hip import abi
    B, H, W = 2, 64, 96
    frame, wt, bias, pre = E.stem_data(cout, H, W, dtype, B)
    want = X.exact_epilogue(pre, 'relu', dtype).cuda()
    g = Guarded(dtype)
    g.tensor(cout, 1, 'front guard')
    dst = g.conv([g.eng.input_id], wt, bias, 3, 2, 'relu', 1)
    g.tensor(12, 1, 'guard before the space-to-depth input')
    g.bind(B, H, W)
    s2d = g.s2d
    guard = max(t for t in g.names if t != s2d)
    assert g.eng.input_id not in g.placed and g.span[s2d][0] == g.up(g.span[guard][1]) and g.up(g.span[s2d][1]) + 256 == g.base + g.need
    g.prepare({}, nan=[s2d])
    tag = 'stem-%d-%dx%d-%s' % (cout, H, W, DT_ID[dtype])
    for xdt in dict.fromkeys((dtype, F32)):
        x = frame.to(xdt).cuda()
        x0 = x.clone()
        wants = [(dst, want), (s2d, _s2d(frame).to(dtype))]
        g.poison()
        g.eng.forward(x)
        g.check(wants, [dst, s2d], tag + ' default, frame ' + DT_ID[xdt])
        g.assert_sensitive([dst, s2d], s2d, dst, tag)
        assert 'generic' in _walk(g, [1], wants, [dst, s2d], GENERIC + PIPE, x, tag, B)
        assert torch.equal(x, x0)
        RECORD.setdefault('input_s2d', set()).add((0, 0))
    if dtype != F32:
        x = frame.to(dtype).cuda()
        ran = _walk(g, [1], [(dst, want)], [dst], [(abi.LP_VARIANT_PIPE_P, 3)], x, tag, B)      # s2d is not allowed: it keeps its NaN
        assert ran.get('planar'), 'the planar stem did not take the op'
        assert torch.isnan(g.full(s2d).float()).all()


@HALF
@pytest.mark.parametrize('c1,c2', [(8, 24), (24, 40), (24, 64)])
def test_fused_stem_writes_only_the_second_layer(c1, c2, dtype):
    """LP_VARIANT_FUSED_STEM2 on the shapes of test_fused_stem_partial_widths: the three separate ops first (three written tensors),
    then the fused form on every tile: only the second layer's destination changes; the stem's tensor and the space-to-depth input
    keep their NaN pre-fill, padding channels included."""
    from yolov6.hip import abi
    B, H, W = 2, 64, 96
    frame, w1, b1, w2, b2, y1, pre2 = E.fused_data('stem', c1, c2, H, W, dtype, B)
    want1, want2 = y1.float().to(dtype).cuda(), X.exact_epilogue(pre2, 'relu', dtype).cuda()
    g = Guarded(dtype, None)
    g.tensor(c1, 1, 'front guard')
    a = g.conv([g.eng.input_id], w1, b1, 3, 2, 'relu', 1)
    d = g.conv([a], w2, b2, 3, 2, 'relu', 2)
    g.tensor(12, 1, 'guard before the space-to-depth input')
    g.bind(B, H, W)
    g.prepare({}, nan=[g.s2d])
    x = frame.to(dtype).cuda()
    tag = 'fused_stem-%d-%d-%dx%d-%s' % (c1, c2, H, W, DT_ID[dtype])
    g.eng.forward(x)
    g.check([(a, want1), (d, want2), (g.s2d, _s2d(frame).to(dtype))], [a, d, g.s2d], tag + ' separate ops')
    ran = _walk(g, [2], [(d, want2)], [d], [(abi.LP_VARIANT_FUSED_STEM2, 3)], x, tag, B)
    if (c1, c2) == (24, 64):
        assert ran.get('fused_stem'), 'the fused stem did not take the op'
    if ran.get('fused_stem'):
        g.assert_sensitive([d], d, d, tag)
        assert torch.isnan(g.full(a).float()).all() and torch.isnan(g.full(g.s2d).float()).all()


@HALF
@pytest.mark.parametrize('c1,c2,h,w', E.FUSED_PW_SHAPES)
def test_fused_1x1_stride2_writes_only_the_second_layer(c1, c2, h, w, dtype):
    """LP_VARIANT_FUSED_PW_S2 on the shapes of test_fused_1x1_stride2_bits: the skipped 1x1 layer's tensor keeps its pre-fill."""
    from yolov6.hip import abi
    B, sl = 2, 3
    x0, w1, b1, w2, b2, y1, pre2 = E.fused_data('pw', c1, c2, h, w, dtype, B)
    want1, want2 = y1.float().to(dtype).cuda(), X.exact_epilogue(pre2, 'relu', dtype).cuda()
    g = Guarded(dtype)
    g.tensor(64, sl, 'front guard')
    src = g.tensor(64, sl, 'src0')
    a = g.conv([src], w1, b1, 1, 1, 'relu', sl)
    d = g.conv([a], w2, b2, 3, 2, 'relu', sl + 1)
    g.bind(B, h << sl, w << sl)
    g.prepare({src: x0})
    x = E._frame(B, h << sl, w << sl)
    inp = g.eng.input_id
    tag = 'fused_pw-%d-%d-%dx%d-%s' % (c1, c2, h, w, DT_ID[dtype])
    g.eng.forward(x)
    g.check([(a, want1), (d, want2)], [inp, a, d], tag + ' separate ops')
    ran = _walk(g, [2], [(d, want2)], [inp, d], [(abi.LP_VARIANT_FUSED_PW_S2, 3)], x, tag, B)
    if c1 == c2:
        assert ran.get('fused_pw'), 'the fused form did not take the op'
    if ran.get('fused_pw'):
        g.assert_sensitive([inp, d], d, d, tag)
        assert torch.isnan(g.full(a).float()).all()


@HALF
def test_bifusion_fused_writes_only_cv3(dtype):
    """LP_VARIANT_FUSED_BIFUSION at (6, 14, B = 2): the three launches first (their bits are the reference, as in
    test_bifusion_fused_equals_its_three_ops), then the fused kernel: only cv3's destination changes, the transposed convolution's and
    cv1's tensors keep their NaN pre-fill."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    h, w, B, sl = 6, 14, 2, 4
    C0, C1, C = 64, 128, 64
    g = Guarded(dtype)
    eng = g.eng
    g.tensor(C0, sl, 'front guard')
    x0, x1, dd = g.tensor(C0, sl, 'src0'), g.tensor(C1, sl - 1, 'src1'), g.tensor(C, sl - 1, 'src2')
    u = g.dest(C, sl - 1)
    wd, bd = _rand((C0, C, 2, 2), 1, (1.0 / C0) ** 0.5), _rand((C,), 2, 0.3)
    abi.check(eng.lib.lp_engine_add_deconv2x2(eng.h, x0, u, eng._ptr(_f32(wd)), eng._ptr(_f32(bd))))
    a = g.conv([x1], _rand((C, C1, 1, 1), 3, (2.0 / C1) ** 0.5), _rand((C,), 4, 0.3), 1, 1, 'relu', sl - 1)
    out = g.conv([u, a, dd], _rand((C, 3 * C, 1, 1), 5, (2.0 / (3 * C)) ** 0.5), _rand((C,), 6, 0.3), 1, 1, 'relu', sl - 1)
    H, W = h << sl, w << sl
    g.bind(B, H, W)
    g.prepare({x0: _rand((B, C0, h, w), 10), x1: _rand((B, C1, 2 * h, 2 * w), 11), dd: _rand((B, C, 2 * h, 2 * w), 12)})
    x = E._frame(B, H, W)
    inp, op = eng.input_id, eng.lib.lp_engine_num_ops(eng.h) - 1
    eng.forward(x)
    g.check([], [inp, u, a, out], 'bifusion: three launches')
    want = eng.tensor_view(out).clone()
    assert not torch.isnan(want.float()).any()
    eng.set_variant(op, abi.LP_VARIANT_FUSED_BIFUSION, 3)
    assert eng.lib.lp_engine_op_carrier(eng.h, 1, 0) == op and eng.lib.lp_engine_op_carrier(eng.h, 2, 0) == op
    for rep in range(2):
        _poison_lds()
        g.poison()
        eng.forward(x)
        g.check([(out, want)], [inp, out], 'bifusion fused, run %d' % rep)
        assert torch.isnan(g.full(u).float()).all() and torch.isnan(g.full(a).float()).all()
    g.assert_sensitive([inp, out], out, out, 'bifusion fused')
    RECORD.setdefault('fused_bifusion', set()).add((0, 0))
    _log('fused_bifusion B=%d %dx%d %s contained' % (B, h, w, DT_ID[dtype]))


# ---- the head ------------------------------------------------------------------------------------------------------------------------
def _carve(pieces, guard=4096):
    """One 0xA5-filled uint8 buffer holding ``pieces`` = [(name, bytes, alignment)] with ``guard`` bytes in front of, between and behind
    them: (buffer, {name: (a, b)}, regions for ByteWatch).  Every piece starts on its alignment in DEVICE addresses."""
    total = guard + sum(n + al + guard for _, n, al in pieces)
    buf = torch.full((total,), POISON, dtype=torch.uint8, device='cuda:0')
    at, regions, off, prev = {}, [], guard, 'the front'
    for name, n, al in pieces:
        a = off + (-(buf.data_ptr() + off)) % al
        regions += [('guard before ' + name, at[prev][1] if prev in at else 0, a), (name, a, a + n)]
        at[name] = (a, a + n)
        off, prev = a + n + guard, name
    regions.append(('guard after ' + prev, at[prev][1], total))
    return buf, at, regions


def _head_engine(dtype, bins, B, H, W, C=64):
    """Levels 3..5 of an H x W input: class and box predictors per level on guarded source maps (the head has no arena destinations)."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    g = Guarded(dtype)
    eng = g.eng
    g.tensor(C, 3, 'front guard')
    feats = [g.tensor(C, 3 + i, 'src%d' % i) for i in range(3)]
    g.tensor(C, 5, 'back guard')
    for i, f in enumerate(feats):
        wc, bc = _rand((277, C), 30 + i, 0.3), _rand((277,), 40 + i, 1.0)
        wb, bb = _rand((4 * bins + 8, C), 50 + i, 0.2), _rand((4 * bins + 8,), 60 + i, 1.0)
        proj = torch.linspace(0, bins - 1, bins)
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, 277, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, i, bins, eng._ptr(_f32(wb)), eng._ptr(_f32(bb)),
                                                 eng._ptr(_f32(proj)) if bins > 1 else None))
    g.bind(B, H, W)
    g.prepare({f: _rand((B, C, H >> (3 + i), W >> (3 + i)), 70 + i) for i, f in enumerate(feats)})
    return g


@ALL3
@pytest.mark.parametrize('bins', [1, 17])
@pytest.mark.parametrize('B', [2, 3])
def test_head_writes_the_whole_prediction_tensor_and_nothing_else(B, bins, dtype):
    """Class predictors (the tiled generic kernel, then the LP_VARIANT_ROWS row writer; tiles straddle images at 12 x 4 anchors) and
    box predictors (plain and DFL) of levels 3..5 of a 128 x 96 input: the prediction tensor is a NaN-filled view inside a larger
    0xA5-filled buffer; all B*N*290 floats are written and equal a plain forward, column 4 is 1, nothing around the view and nothing
    in the arena but the network input changes."""
    H, W = 128, 96
    g = _head_engine(dtype, bins, B, H, W)
    eng = g.eng
    x = E._frame(B, H, W)
    plain = eng.forward(x).clone()
    N = eng.n_anchors
    assert N == 16 * 12 + 8 * 6 + 4 * 3 and plain.shape == (B, N, 290) and not torch.isnan(plain).any()
    buf, at, regions = _carve([('pred', B * N * 290 * 4, 16)])
    pred = buf[at['pred'][0]:at['pred'][1]].view(torch.float32).view(B, N, 290)
    eng._new_pred = lambda n: pred                               # the engine's forward writes into the guarded view
    for form in ('tiled', 'rows', 'tiled again'):
        for op in (1, 3, 5):
            eng.set_variant(op, *((18, 1) if form == 'rows' else (2, 1)))
        pred.fill_(NAN)
        watch = X.ByteWatch(buf, regions)
        g.watch.snapshot()
        assert eng.forward(x) is pred
        tag = 'head-%s-B%d-bins%d-%s' % (form, B, bins, DT_ID[dtype])
        g.check([], [eng.input_id], tag)                             # the arena: only the network input is written
        watch.assert_contained([at['pred']], tag)
        assert torch.equal(pred, plain), tag                         # every float written (a NaN is equal to nothing)
        assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))
        r = watch.report([(at['pred'][0] + 16, at['pred'][1] - 16)])
        cur, snap = buf.cpu().numpy(), watch.snap.cpu().numpy()
        ends = list(range(at['pred'][0], at['pred'][0] + 16)) + list(range(at['pred'][1] - 16, at['pred'][1]))
        assert r['offsets'].tolist() == [o for o in ends if cur[o] != snap[o]] and r['count'] >= 8
        assert [reg[0] for reg in r['regions']] == ['pred']
        RECORD.setdefault('head_' + form.split()[0], set()).add((0, 0))
        _log('head_%s B=%d bins=%d %s contained' % (form.split()[0], B, bins, DT_ID[dtype]))


@ALL3
@pytest.mark.parametrize('bins', [1, 17])
def test_detections_only_forward_writes_only_its_workspace(bins, dtype):
    """lp_engine_forward_det with a workspace of exactly lp_nms_workspace_bytes inside a guarded buffer: nothing around the workspace
    changes; in the arena only the network input and what lies behind the tensors (the prediction scratch of levels whose class
    predictors do not fit the row kernel) may change.  Inside the workspace the candidate rows of anchors that do NOT pass the
    confidence mask keep their pre-fill as far as lp_hip.h says: columns 12..27 always (the class kernels append passing anchors
    only), columns 0..11 too while the box predictors run in the sparse form (the default without DFL); in the dense form
    (LP_VARIANT_BOX_DENSE, and DFL heads, whose box predictors go through the generic decode kernel) columns 0..11 of EVERY anchor's
    row are written.  lp_nms_candidates then gives the bits of lp_nms on a plain forward."""
    from yolov6.hip import abi, runtime
    B, H, W = 2, 128, 96
    g = _head_engine(dtype, bins, B, H, W)
    eng = g.eng
    x = E._frame(B, H, W)
    plain = eng.forward(x)
    N = eng.n_anchors
    cf = torch.stack([plain[..., a:b].max(-1).values for a, b in zip(X.SEG[:-1], X.SEG[1:])], -1)
    mask = (cf[..., :7].sum(-1) + cf[..., 6]) / 8.0
    conf = float(mask.median())
    assert 0.0 < conf < 1.0
    det2, count2, keep2 = runtime.nms_padded(plain.clone(), conf, 0.45, 300, want_keep=True)
    need = eng.lib.lp_nms_workspace_bytes(B, N)
    buf, at, regions = _carve([('workspace', need, 256)])
    a, b = at['workspace']
    scratch = [r[1:] for r in g.regions if r[0] == 'behind the tensors']
    forms = [('sparse', abi.LP_VARIANT_BOX_SPARSE), ('dense', abi.LP_VARIANT_BOX_DENSE)] if bins == 1 else [('generic decode', None)]
    for form, variant in forms:
        if variant is not None:
            for op in (2, 4, 6):
                eng.set_variant(op, variant, 1)
        buf.fill_(POISON)
        watch = X.ByteWatch(buf, regions)
        g.watch.snapshot()
        abi.check(eng.lib.lp_engine_forward_det(eng.h, ctypes.c_void_p(x.data_ptr()), abi.LP_F32, conf, ctypes.c_void_p(buf.data_ptr() + a),
                                                need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lp_engine_forward_det')
        tag = 'forward_det-bins%d-%s-%s' % (bins, form.split()[0], DT_ID[dtype])
        watch.assert_contained([(a, b)], tag)
        g.watch.assert_contained(g.allowed([eng.input_id]) + scratch, tag)
        ws = buf[a:b]
        cnt, keys, rows = X.det_workspace_views(ws, B, N)
        n = cnt.cpu().tolist()
        assert all(0 < k < N for k in n), n
        failed = torch.ones(B, N, dtype=torch.bool, device='cuda:0')
        for i in range(B):
            failed[i, (keys[i, :n[i]] & 0xffffffff).long()] = False
        stale = rows.view(torch.int32)[failed] != -1515870811            # 0xA5A5A5A5: the pre-fill
        box, cls = int(stale[:, :12].sum()), int(stale[:, 12:].sum())
        _log('forward_det %s candidates=%s, rows of the %d anchors that did not pass: %d box elements and %d class elements changed'
             % (tag, n, stale.shape[0], box, cls))
        assert cls == 0, tag
        assert box == (0 if form == 'sparse' else 12 * stale.shape[0]), tag
        det, count, keep = runtime.nms_candidates((ws, B, N), 0.45, 300, want_keep=True)
        assert torch.equal(count, count2) and torch.equal(keep, keep2) and torch.equal(det, det2) and int(count.min()) > 0, tag
    RECORD.setdefault('forward_det', set()).add((0, 0))


# ---- D. lp_nms / lp_nms_candidates through the ABI ---------------------------------------------------------------------------------
def _nms_guarded(pred_np, conf, iou, max_det, tag):
    """lp_nms, then lp_nms_candidates on the workspace it left, with pred, det, count, keep and a workspace of exactly
    lp_nms_workspace_bytes as views inside one guarded buffer; both against the C oracle: bit-equal kept indices and rows, rows past
    the count zero, keep -1 there, pred changed as the oracle's copy, no guard byte changed.  -> the oracle's (rows, keep)."""
    from oracle import lp_post
    from yolov6.hip import abi
    lib = abi.load()
    B, N, _ = pred_np.shape
    rows_o, keep_o, after = lp_post.nms_c(pred_np, conf, iou, max_det)
    need = lib.lp_nms_workspace_bytes(B, N)
    buf, at, regions = _carve([('pred', pred_np.nbytes, 16), ('det', B * max_det * 28 * 4, 16), ('count', 4 * B, 4), ('keep', 4 * B * max_det, 4),
                               ('workspace', need, 256)])
    view = lambda name, dt: buf[at[name][0]:at[name][1]].view(dt)
    pred, det, count, keep = view('pred', torch.float32), view('det', torch.float32).view(B, max_det, 28), view('count', torch.int32), \
        view('keep', torch.int32).view(B, max_det)
    ptr = lambda name: ctypes.c_void_p(buf.data_ptr() + at[name][0])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pred.copy_(torch.from_numpy(pred_np).reshape(-1))
    watch = X.ByteWatch(buf, regions)
    for entry in ('lp_nms', 'lp_nms_candidates'):
        if entry == 'lp_nms':
            abi.check(lib.lp_nms(ptr('pred'), B, N, conf, iou, max_det, ptr('det'), ptr('count'), ptr('keep'), ptr('workspace'), need, st), entry)
            allowed = [at[k] for k in ('pred', 'det', 'count', 'keep', 'workspace')]
        else:
            for name in ('det', 'count', 'keep'):
                buf[at[name][0]:at[name][1]] = POISON
            watch.snapshot()
            abi.check(lib.lp_nms_candidates(B, N, iou, max_det, ptr('det'), ptr('count'), ptr('keep'), ptr('workspace'), need, st), entry)
            allowed = [at[k] for k in ('det', 'count', 'keep', 'workspace')]
        watch.assert_contained(allowed, '%s %s' % (entry, tag))
        n, d, k = count.cpu().numpy(), det.cpu().numpy(), keep.cpu().numpy()
        for i in range(B):
            assert n[i] == len(rows_o[i]), (entry, tag, i, n[i], len(rows_o[i]))
            assert np.array_equal(k[i, :n[i]], keep_o[i]) and np.array_equal(d[i, :n[i]].view(np.int32), rows_o[i].view(np.int32)), (entry, tag, i)
            assert not d[i, n[i]:].view(np.int32).any() and (k[i, n[i]:] == -1).all(), (entry, tag, i)
        assert np.array_equal(pred.cpu().numpy().view(np.int32), after.reshape(-1).view(np.int32)), (entry, tag)
    # the checker notices: the first granule of det and the last of keep were written by the launch
    r = watch.report([at['workspace'], at['count'], (at['det'][0] + 16, at['det'][1]), (at['keep'][0], at['keep'][1] - 16)])
    cur, snap = buf.cpu().numpy(), watch.snap.cpu().numpy()
    ends = list(range(at['det'][0], at['det'][0] + 16)) + list(range(at['keep'][1] - 16, at['keep'][1]))
    assert r['offsets'].tolist() == [o for o in ends if cur[o] != snap[o]] and r['count'] >= 8, r
    assert [reg[0] for reg in r['regions']] == ['det', 'keep']
    _log('nms %s kept=%s contained' % (tag, [len(v) for v in keep_o]))
    return rows_o, keep_o


NMS_CASES = [
    # (B, N, share of anchors with a high score, obj == 1, conf, iou, max_det)
    (2, 77, 1.0, True, 0.30, 0.10, 1000),
    (1, 1024, 1.0, True, 0.03, 0.45, 300),            # 1024 candidates: an exact power of two and exactly one staged batch
    (1, 1025, 1.0, True, 0.03, 0.45, 300),            # one candidate in the second batch
    (3, 2100, 0.2, False, 0.25, 0.5, 50),             # obj != 1: the prediction tensor is modified in place
]


@pytest.mark.parametrize('case', NMS_CASES, ids=lambda c: 'B%d-N%d-conf%g-iou%g-max%d' % (c[0], c[1], c[4], c[5], c[6]))
def test_nms_writes_only_its_buffers(case):
    B, N, hot, obj_one, conf, iou, max_det = case
    pred = X.synth_pred(B, N, 40 + N, frac_hot=hot, obj_one=obj_one).numpy()
    rows, keep = _nms_guarded(pred, conf, iou, max_det, 'B%d-N%d' % (B, N))
    if hot == 1.0 and conf <= 0.03:
        r = X.post64_rows(pred[0])
        assert int((r['mask'].astype(np.float32) >= np.float32(conf)).sum()) == N      # every anchor is a candidate
    assert sum(len(k) for k in keep) > 0


# ---- E. suppression through the spilled kept list ------------------------------------------------------------------------------------
@pytest.mark.parametrize('first_rank,n_copy', [(4100, 1900), (4000, 2000)], ids=['beyond-the-cache', 'straddling-the-cache'])
def test_suppression_by_kept_boxes_beyond_the_lds_cache(first_rank, n_copy):
    """greedy_kernel caches the first 4096 kept boxes in LDS; with max_det = 8000 (> 4032) the list spills to global memory.  6000
    disjoint boxes in descending score order, all kept, then lower-scored copies (IoU 56 / 72 with their original, disjoint from
    everything else) of the boxes ranked ``first_rank`` onwards: every copy can only be suppressed by ONE kept box, whose kept rank is
    beyond the cache (first case; 1900 copies: 6000 originals leave no room for 2000 of them past rank 4096) or on either side of the
    boundary (second case, 2000 copies, N = 8000).  The preconditions come from the C oracle and float64 geometry alone
    (lp_testing.assert_spill_preconditions, also run on the CPU); then lp_nms is bit-equal to the oracle."""
    p, box, score = X.spill_case(first_rank, 6000, n_copy)
    _, _, orig = X.assert_spill_preconditions(p, box, score, first_rank, 6000, n_copy, 0.25, 0.5, 8000)
    assert orig.min() >= 4096 if first_rank >= 4096 else (orig.min() < 4096 <= orig.max())
    rows, keep = _nms_guarded(p, 0.25, 0.5, 8000, 'spill-from-rank-%d' % first_rank)
    assert len(keep[0]) == 6000


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def test_every_family_of_the_exact_tests_was_checked_on_two_tiles():
    """Every kernel family the exact tests exercise was also checked for containment: generic, PIPE, PIPE16, PIPE16_V, S2P16, the planar
    stem, the fused stem and the fused 1x1 + stride-2 form on at least two distinct tiles each, the streaming 1x1 kernel (no tiles) at
    all.  Self-contained: one case per family is run again here and the record of what was checked is counted."""
    RECORD.clear()
    pick = lambda key: next(c for c in A_CASES if c[1:7] == key)
    test_conv_families_write_only_their_destinations(pick(((64,), 96, 3, 1, 33, 17)), F16)       # generic, PIPE, PIPE16, PIPE16_V
    test_conv_families_write_only_their_destinations(pick(((128,), 128, 3, 1, 20, 20)), F16)     # the same four
    test_conv_families_write_only_their_destinations(pick(((96,), 200, 3, 2, 34, 22)), F16)      # S2P16
    test_conv_families_write_only_their_destinations(pick(((256,), 128, 1, 1, 20, 20)), F16)     # stream
    test_stem_and_space_to_depth_input(24, F16)                                                  # planar
    test_fused_stem_writes_only_the_second_layer(24, 64, F16)
    test_fused_1x1_stride2_writes_only_the_second_layer(64, 64, 40, 56, F16)
    assert RECORD.get('stream'), sorted(RECORD)
    few = {f: sorted(RECORD.get(f, ())) for f in ('generic', 'PIPE', 'PIPE16', 'PIPE16_V', 'S2P16', 'planar', 'fused_stem', 'fused_pw')
           if len(RECORD.get(f, ())) < 2}
    assert not few, few
    with open(os.path.join(X.log_dir(), LOG_NAME)) as f:
        logged = {line.split(':')[0] for line in f}
    assert {'generic', 'stream', 'PIPE', 'PIPE16', 'PIPE16_V', 'S2P16', 'planar', 'fused_stem', 'fused_pw'} <= logged
