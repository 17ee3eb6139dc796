"""The extractor's kernels get their dynamic-LDS attributes from their own translation unit's once-flag (csrc/conv.hip ext_cfg), the MIL kernels from
theirs (csrc/gemm_f32.hip cfg). Which library call comes first in a process therefore decides what has run before a launch - and the suite, one
process in a fixed order, cannot see that. Each case here starts ONE fresh process whose first launching call is one extractor operation
(tests/_extractor_first_call_probe.py) and which checks the result as the operation's own test in tests/test_resnet_extractor.py does. A missing
attribute is a launch error -> RuntimeError in the child -> a non-zero exit status here."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(REPO, "tests", "_extractor_first_call_probe.py")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stem_pool_nchw",     # stem_halo_pool_kernel (SH_SMEM)
                                  "conv_nhwc",          # conv3x3_h2_halo_kernel (160 KB)
                                  "linear_wide"])       # ext_linear's wide route: the MIL unit's 256x256 kernel before that unit served any call of its own
def test_extractor_operation_as_the_first_call_of_a_process(cuda, case):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [PROBE, case]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert f"FIRST_CALL_PROBE {case} ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])       # (linear_wide: the child asserted toad_fallback_launches() == 0)
