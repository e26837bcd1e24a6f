"""CPU test of the kernel selection rules (pick_cfg, conv_pipe_fits, op_fam16 in the library's host code): which kernel families
take a 3x3 layer at the edges of the kernels' LDS tables, and which one the rule makes the default at finalize.  One-conv engines on
the CPU: without a bound arena lp_engine_set_op_variant only applies the rule.  The rows (lp_testing.RULE_ROWS) are run on the
GPU, every family that takes them, in test_exact_edges_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import lp_testing as X
from test_exact_gpu import ALL_VARIANTS, _family

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def one_conv_engine(dtype, cins, cout, stride, device='cpu'):
    """Input op + one 3x3 layer over ``cins`` (zero weights), production default of the MFMA family; the layer is op 1."""
    from yolov6.hip import abi, runtime
    eng = runtime.Engine(dtype, device, mfma16=None)
    srcs = [eng.tensor(c, 3) for c in cins]
    eng.conv(srcs, np.zeros((cout, sum(cins), 3, 3), np.float32), np.zeros(cout, np.float32), 3, stride, abi.LP_ACT_RELU, 3)
    return eng.finish()


def default_family(eng, op=1):
    from yolov6.hip import abi
    cfg = ctypes.c_int()
    abi.check(eng.lib.lp_engine_op_variant(eng.h, op, ctypes.byref(cfg), None), 'lp_engine_op_variant')
    return _family(cfg.value)


def accepting_families(eng, op=1):
    took = set()
    for cfg, nb in ALL_VARIANTS:
        try:
            eng.set_variant(op, cfg, nb)
            took.add(_family(cfg))
        except RuntimeError:
            pass
    return took


@pytest.fixture(autouse=True)
def _production_switches(monkeypatch):
    for name in ('LP_NO_MFMA16', 'LP_S2P16', 'LP_TUNE_CFG128', 'LP_TUNE_NBUF'):       # read when an engine is created / finalized
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('row', X.RULE_ROWS, ids=[r[0] for r in X.RULE_ROWS])
def test_rule_table(row, dtype):
    """The exact set of families whose variants the rule accepts for the layer, and the family of its default."""
    name, cins, cout, stride, pipelined, default = row
    eng = one_conv_engine(dtype, cins, cout, stride)
    assert default_family(eng) == default                                   # (read before any variant is asked for)
    assert accepting_families(eng) == {'generic'} | pipelined, name


@pytest.mark.parametrize('row', X.RULE_ROWS, ids=[r[0] for r in X.RULE_ROWS])
def test_rule_table_fp32_takes_no_pipelined_kernel(row):
    name, cins, cout, stride, _, _ = row
    eng = one_conv_engine(F32, cins, cout, stride)
    assert default_family(eng) == 'generic'
    assert accepting_families(eng) == {'generic'}, name
