"""The fp16 build of csrc/mlp_bf16_16.hip (-DNERF_HALF) runs the FOLDED layer table: its MFMA count is the unfolded
one less layers_2's, and the hazard-nop budget of the bf16 build (tests/test_library_cpu.py) holds for it too.
Needs hipcc like its sibling; no GPU."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the schedule's own arithmetic, from the layout constants of csrc/nerf_layout.h ------------------------------------
# (layer: output rows padded to 16-row tiles, padded K); a wave owns two 16-point column blocks and one MFMA
# (16 rows x 16 points x 32 k) per (row tile, k-step of 32, column block)
ROWS_K = {0: (256, 64), 1: (256, 256), 2: (256, 256), 3: (256, 256), 4: (256, 256), 5: (256, 320), 6: (256, 256),
          7: (256, 256), 8: (256 + 16, 256), 9: (128, 288), 10: (16, 128)}
NCB = 2


def mfmas(rows_k):
    return sum(rows // 16 * (k // 32) * NCB for rows, k in rows_k.values())


UNFOLDED = mfmas(ROWS_K)
LAYERS_2 = 256 // 16 * (256 // 32) * NCB                         # 16 row tiles x 8 k-steps x 2 column blocks
# folded: layer 8 keeps its sigma tile as a one-tile layer (nothing added), the colour layer keeps its shape
FOLDED_ROWS_K = {**ROWS_K, 8: (16, 256)}
FOLDED = mfmas(FOLDED_ROWS_K)


def chunks(rows_k):
    """weight chunks per tile: four 16-row tiles per chunk, eight for the K = 64 first layer"""
    return sum(-(-(rows // 16) // (8 if L == 0 else 4)) for L, (rows, k) in rows_k.items())


def test_schedule_arithmetic():
    assert UNFOLDED == 2344 and LAYERS_2 == 256                  # what test_inference_kernels_have_few_hazard_nops pins
    assert FOLDED == UNFOLDED - LAYERS_2
    assert chunks(ROWS_K) == 38 and chunks(FOLDED_ROWS_K) == 34 and chunks(FOLDED_ROWS_K) % 2 == 0     # buffer parity
    # 16 rows x 16 points x 32 k per MFMA, 32 points per wave: padded MACs per point
    assert UNFOLDED * 16 * 16 * 32 // 32 == 600064 and FOLDED * 16 * 16 * 32 // 32 == 600064 - 65536


def test_fp16_inference_kernels_run_the_folded_schedule():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_vmcnt
    finally:
        sys.path.pop(0)
    asm = check_vmcnt.assemble(os.path.join(ROOT, "nerf-simple_amd", "csrc", "mlp_bf16_16.hip"), extra=("-DNERF_HALF",))
    kernels = check_vmcnt.kernels_of(asm)
    assert len(kernels) == 3, list(kernels)                      # fp16 has no training forward
    for name, body in kernels.items():
        assert "nerf_mlp_f16_16_kernel" in name, name
        lines = body if isinstance(body, list) else body.split("\n")
        mfma = [i for i, ln in enumerate(lines) if re.match(r"\s+v_mfma", ln)]
        assert len(mfma) == FOLDED, (name, len(mfma))
        assert all("16x16x32_f16" in lines[i] for i in mfma), name
        nops = [ln for ln in lines[mfma[0]:mfma[-1] + 1] if re.match(r"\s+s_nop", ln)]
        assert len(nops) <= 150, (name, len(nops))
    # the counted waits in front of the chunk barriers: one per chunk of the folded schedule and the launch's own
    for name, (checked, bad) in {k: check_vmcnt.check_kernel(v) for k, v in kernels.items()}.items():
        assert checked == chunks(FOLDED_ROWS_K) + 1 and not bad, (name, checked, bad[:5])
    # the fused render keeps the name bench.py looks its counters up by
    assert any("nerf_mlp_f16_16_kernelILb1ELb0ELb1EE" in k for k in kernels)
