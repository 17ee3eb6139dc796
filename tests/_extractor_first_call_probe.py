"""Helper for tests/test_gpu_extractor_first_call.py: a fresh process whose FIRST call into libtoad_hip.so that launches anything is ONE extractor
operation, so that the only kernel attributes set before its launch are those of its own translation unit's initialiser (csrc/conv.hip ext_cfg; the
wide route: csrc/gemm_f32.hip cfg, reached through the extractor's launcher). The check of the result is the existing test of that operation in
tests/test_resnet_extractor.py, called as a function on the one shape: same data recipe, same comparison, same tolerance.
    python tests/_extractor_first_call_probe.py stem_pool_nchw | conv_nhwc | linear_wide"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tests import test_resnet_extractor as checks
from toad_amd import _lib

case = sys.argv[1]
cuda = torch.device("cuda:0")
lib = _lib.load()
if case == "stem_pool_nchw":        # tiles (1, 3, 4, 256): stem_halo_pool_kernel, SH_SMEM of dynamic LDS
    checks.test_stem_and_pool_straight_from_nchw_tiles(cuda, 1, 4)
elif case == "conv_nhwc":           # 3x3 / 1 / 1 on (1, 16, 16, 64) -> 64 channels, M = 256: conv3x3_h2_halo_kernel, 160 KB
    checks.test_implicit_conv_matches_fp64(cuda, 1, 16, 16, 64, 64, 3, 1, 1, False)
elif case == "linear_wide":         # M = 256, K = 128, N = 512, no residual: the extractor's launcher into the MIL unit's 256x256 kernel
    checks.test_linear_act_res_matches_fp64(cuda, 256, 128, 512, False, 1)
    assert lib.toad_fallback_launches() == 0, "the wide route fell back to the exact-fp32 kernel"
else:
    raise SystemExit(f"unknown case {case!r}")
torch.cuda.synchronize()
print(f"FIRST_CALL_PROBE {case} ok fallback_launches={lib.toad_fallback_launches()}", flush=True)
