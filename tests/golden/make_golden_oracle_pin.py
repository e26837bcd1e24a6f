"""SHA-256 digests of the forward oracle's default (fp32) outputs on the tiny golden cases, recorded with the oracle as it stood
BEFORE it gained its ``precision`` argument (tests/golden/oracle_fp32_pin.npz): tests/test_e2e_cpu.py asserts that the default
path still gives these bits.  bench.py's CPU baseline and smoke() run that path.  Recorded with 4 ATen threads, like the other
fixtures.

    python tests/golden/make_golden_oracle_pin.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

from conftest import load_golden  # noqa: E402
from oracle import lp_oracle  # noqa: E402

PIN_CASES = [('lps_tiny_128x96', 'lps_tiny_weights', 'yololps', None), ('lps_tiny_64x160', 'lps_tiny_weights', 'yololps', None),
             ('v6m_tiny_96x128', 'v6m_tiny_weights', 'yolov6m', None),
             ('lps_tiny_128x96', 'lps_tiny_weights', 'yololps', torch.float16), ('v6m_tiny_96x128', 'v6m_tiny_weights', 'yolov6m', torch.bfloat16)]


def digests(case, weights, name, round_to):
    """[pred, neck0, neck1, neck2] -> hex digests of the raw fp32 bytes."""
    g, sd = load_golden(case), load_golden(weights)
    x = g['x'] if round_to is None else g['x'].to(round_to)
    pred, neck = lp_oracle.forward(sd, lp_oracle.arch(name, width=0.0625), x, round_to=round_to)
    assert pred.dtype == torch.float32
    return [hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() for t in [pred] + list(neck)]


def pin_key(case, round_to):
    return case + ('' if round_to is None else '_' + str(round_to).split('.')[-1])


if __name__ == '__main__':
    torch.set_num_threads(4)
    out = {pin_key(c, r): np.array(digests(c, w, n, r)) for c, w, n, r in PIN_CASES}
    np.savez(os.path.join(HERE, 'oracle_fp32_pin.npz'), **out)
    for k, v in out.items():
        print(k, v[0][:16])
