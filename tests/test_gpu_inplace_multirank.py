"""In-place activated SyncBatchNorm on two ranks sharing cuda:0 (gloo group,
the mechanism of test_gpu_multirank.py, through ``multirank_harness``): bf16
channels-last, LeakyReLU(0.2), against the float64 oracle of the whole batch.

The case function, its data and its bounds are those of the CPU tier
(tests/test_inplace_abn.py::run_rank_case): statistics, coefs and running
statistics against ``oracle64`` of the whole x with
test_gpu_reduction_edges' ``_check_*`` bounds, y and dx with ``_tol(bf16)``,
the rank's grad_weight / grad_bias with the derived summation bounds against
``inplace_oracle`` of the whole batch's stored y.
"""

import pytest
import torch

import multirank_harness as harness

pytestmark = pytest.mark.gpu


def test_inplace_sync_world2_gpu(tmp_path):
    # (name, per-rank sizes, C, plane, dtype, channels_last, seed)
    case = ("bf16_nhwc", (4, 4), 16, (6, 6), torch.bfloat16, True, 61)
    outputs = harness.run_cases(tmp_path, 2, "cuda:0",
                                "test_inplace_abn:run_rank_case", [case])
    assert sorted(outputs) == [0, 1]
    for rank, per_case in outputs.items():
        for _, text in per_case:
            print(text, end="")
            for q in ("mean", "invstd", "scale", "y", "grad_weight", "dx"):
                assert f"] {q}:" in text, (rank, q)
