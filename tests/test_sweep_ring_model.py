"""CPU check of the persistent ring of zs_k_sweep (deflate_sweep.hip, levels
4..6): tools/emu/emu_sweep_ring.c replays, with the functions of
csrc/zs_sweep_ring.h that the kernel itself calls, the ring writes and reads of
16 waves claiming runs of chunks from a shared counter.  For every chain (16,
32, 128), run cap (1, 2, 8, 16), pattern of skipped chunks (none, the first half,
the last third, alternating, one in three) and pattern of chunks whose sweep
goes past step 64 (never, always, alternating, in pairs), every slot a step
reads -- single slots, groups read upwards from their lowest slot through the
mirror, and the member positions read after the sweep -- must hold the
member the step means, written in the wave's current run.  No GPU needed; the
kernel's results are checked by tests/test_gpu_sweep_runs.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_sweep_ring.c")

MEMBERS = [1, 63, 64, 65, 127, 128, 129, 192, 193, 511, 512, 513, 577, 65534]
CASES = 3 * 4 * 5 * 4  # chains x run caps x skip patterns x past-64 patterns


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_sweep_ring")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    return exe


@pytest.mark.parametrize("m", MEMBERS)
def test_ring_reads_find_their_members(emu, m):
    r = subprocess.run([emu, str(m)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "m %d: %d cases," % (m, CASES) in r.stdout, r.stdout
    assert "bad reads 0 in 0 cases" in r.stdout, r.stdout


@pytest.mark.parametrize("m", [65, 577])
def test_model_reports_a_missing_mirror(emu, m):
    """The check can fail: without the second copy of slots 0..63 at 192..255 the steps that read past slot 191 are caught."""
    r = subprocess.run([emu, str(m), "break"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "bad reads 0 in" not in r.stdout, r.stdout
