"""CPU side of the batched image identities: the default NullInverter.invert_batch seam and the harness's argument contract."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_invert_batch_loops_over_invert_in_order():
    from diffusionhandles_amd.null_inverter import NullInverter

    class Recorder(NullInverter):
        def __init__(self):
            super().__init__(model=None)
            self.calls = []

        def invert(self, target_img, depth, prompt, num_inner_steps=10, early_stop_epsilon=1e-5, verbose=False, **kw):
            self.calls.append((target_img, depth, prompt, num_inner_steps, early_stop_epsilon, kw))
            return ((target_img, None), f"noise-{prompt}", f"uncond-{prompt}")

    inv = Recorder()
    out = inv.invert_batch(["i0", "i1", "i2"], ["d0", "d1", "d2"], ["p0", "p1", "p2"], num_inner_steps=5)
    assert [o[1] for o in out] == ["noise-p0", "noise-p1", "noise-p2"]
    assert inv.calls == [(f"i{b}", f"d{b}", f"p{b}", 5, 1e-5, {}) for b in range(3)]
    inv.calls.clear()
    inv.invert_batch(["i0"], ["d0"], ["p0"], max_timesteps=3)
    assert inv.calls[0][-1] == {"max_timesteps": 3}
    with pytest.raises(ValueError):
        inv.invert_batch(["i0", "i1"], ["d0"], ["p0", "p1"])


def test_harness_identity_batch_needs_a_test_set():
    tool = os.path.join(ROOT, "tools", "run_edit.py")
    for extra in (["--identity-batch", "2"], ["--identity-batch", "0", "--test-set", "x.json"]):
        r = subprocess.run([sys.executable, tool, *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--identity-batch" in r.stderr, r.stderr[-500:]
