"""The MFMA-shape micro-benchmark (scripts/micro/mfma_shape.hip) compares v_mfma_f32_32x32x16_bf16 with v_mfma_f32_16x16x32_bf16;
the comparison is only as good as its timed loops are clean (an earlier one, mfma_peak16.hip, carried three v_accvgpr moves per
MFMA and measured those).  No GPU needed: the audit compiles the file to ISA and lists each timed loop's instructions."""
import os
import re
import subprocess


def test_mfma_shape_microbenchmark_loops_hold_matrix_instructions_only():
    """scripts/micro/mfma_shape_audit.sh: per kernel, the loop body holds the 16 (32x32x16) or 32 (16x16x32) MFMAs of a 64 x 64 x 64
    wave tile, loop control, and - in the *_lds kernels only - 16 ds_read_b128 and 2 s_waitcnt; no v_accvgpr_* and no other VALU
    or memory instruction; over the whole kernel no compiler value in an accumulation register the asm owns; a failed compile fails."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MFMA_SHAPE_AUDIT_DIR=os.path.join(root, "realtime_video_amd", "csrc", "build", "mfma_shape_audit"))
    run = subprocess.run([os.path.join(root, "scripts", "micro", "mfma_shape_audit.sh")], capture_output=True, text=True, env=env,
                         timeout=600)
    out = run.stdout
    assert run.returncode == 0, out + run.stderr
    for kernel, mfma, reads, waits in (("mfma32_reg", 16, 0, 0), ("mfma16_reg", 32, 0, 0), ("mfma32_lds", 16, 16, 2), ("mfma16_lds", 32, 16, 2)):
        pat = rf"AUDIT {kernel}: loop lines \d+-\d+ mfma {mfma} ds_read_b128 {reads} s_waitcnt {waits} scalar [1-4] v_accvgpr 0 other_valu 0 other 0 compiler_acc_refs 0\b"
        assert re.search(pat, out), out
