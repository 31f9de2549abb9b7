"""CPU check of how zs_k_sweep (deflate_sweep.hip, fold) picks among the long
candidates of a group of eight chain steps: tools/emu/emu_sweep_long.c replays,
with the functions of csrc/zs_sweep_long.h that the kernel itself calls, every
mask of long steps (256), lengths from {10, 11, 13, 14, nice - 1, nice,
nice + 1, 258} clamped by maxc in {13, 14, 258}, nice in {16, 32, 128, 258} and
an incoming best below, at and above the group's, and compares the best long
candidate kept (its length capped at nice, its step) with the reference's serial
walk of the steps in order (first strictly longer, the walk ends at the first
nice one).  Both of the kernel's forms are replayed: all long steps joined in
turn, and the first long step taken from the group's maximum score with the
others joined after it.  No GPU needed; the kernel's results are checked by
tests/test_gpu_sweep_long.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_sweep_long.c")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_sweep_long")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    return exe


def test_long_selection_equals_the_serial_walk(emu):
    r = subprocess.run([emu], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"cases (\d+), bad (\d+)", r.stdout)
    assert m, r.stdout
    # 4 nice x 3 maxc x 9 incoming x 256 masks, two forms each, at least one assignment per mask
    assert int(m.group(1)) >= 4 * 3 * 9 * 256 * 2, r.stdout
    assert int(m.group(2)) == 0, r.stdout


def test_model_reports_a_missing_nice_cap(emu):
    """The check can fail: without the cap at nice a later, longer candidate displaces the first nice one."""
    r = subprocess.run([emu, "break"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    m = re.search(r"cases (\d+), bad (\d+)", r.stdout)
    assert m and int(m.group(2)) > 0, r.stdout
