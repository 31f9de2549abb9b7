"""CPU check of the rule by which zs_k_sweep (deflate_sweep.hip, SwWave::ends) keeps the
unmasked maximum of a group of eight chain steps in which some lane's chain ends:
tools/emu/emu_sweep_ends.c replays whole streams wave by wave and group by group with the
functions of csrc/zs_sweep_ends.h that the kernel itself calls, once with every dead step's
score zeroed (what such a group did before) and once unmasked + rule, and after every group
the lanes' thr, bt, lthr, lbt, liveness and chain >> 2 snapshots must be equal.  Streams: T-, M-
and R-corpus at 64 KiB and the constructed ones of tests/sweependscases.py, at the chain budgets
of levels 5, 6, 7 and 9.  The model also reports the groups per chunk (fast, ends, keys read,
failed validation) that the kernel's -DZS_SW_PROF=1 counters measure.  No GPU needed; the
kernel's bytes are checked by tests/test_gpu_sweep_ends.py."""
import os
import re
import shutil
import struct
import subprocess

import pytest

import corpus
import sweependscases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_sweep_ends.c")
LEVELS = {5: (32, 32), 6: (128, 128), 7: (256, 128), 9: (4096, 258)}  # (chain, nice), deflate.ts:84-100


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_sweep_ends")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    return exe


def _blob(streams):
    return struct.pack("<I", len(streams)) + struct.pack("<%dI" % len(streams), *map(len, streams)) + b"".join(streams)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ends")
    corp = [corpus.text(corpus.stream_seed(0), 65536), corpus.text(corpus.stream_seed(1), 65536),
            corpus.mixed(corpus.stream_seed(2), 65536), corpus.mixed(corpus.stream_seed(3), 65536),
            corpus.rand(corpus.stream_seed(4), 65536), corpus.text(corpus.stream_seed(5), 65537)]
    made = sweependscases.streams()
    out = {"corpus": d / "corpus.bin", "made": d / "made.bin", "text": d / "text.bin"}
    out["corpus"].write_bytes(_blob(corp))
    out["made"].write_bytes(_blob([made[k] for k in sorted(made)]))
    out["text"].write_bytes(_blob(corp[:2]))
    for k in sorted(made):  # one file per constructed stream: each case must occur in its own
        out[k] = d / (k.replace("+", "_") + ".bin")
        out[k].write_bytes(_blob([made[k]]))
    return out


def _run(emu, f, level, *more):
    chain, nice = LEVELS[level]
    r = subprocess.run([emu, str(f), str(chain), str(nice), *more], capture_output=True, text=True, timeout=600)
    m = re.search(r"chunks (\d+), groups (\d+), mismatches (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    rates = dict(zip(("fast", "ends", "keys", "failed", "opart", "okeys", "ofailed", "steps"),
                     map(float, re.search(r"fast ([\d.]+), ends ([\d.]+) \(keys read ([\d.]+), failed ([\d.]+)\); opening "
                                          r"group: partial ([\d.]+), keys read ([\d.]+), failed ([\d.]+); lock-step steps ([\d.]+)",
                                          r.stdout).groups())))
    u = re.search(r"unsettled lanes: dead winner (\d+), long (\d+)", r.stdout)
    return r, int(m.group(3)), rates, (int(u.group(1)), int(u.group(2)))


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_rule_equals_masking_on_corpus_streams(emu, files, level):
    r, bad, rates, _ = _run(emu, files["corpus"], level)
    assert r.returncode == 0 and bad == 0, r.stdout + r.stderr
    assert rates["ends"] > 0 and rates["failed"] <= rates["ends"], r.stdout


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_rule_equals_masking_on_constructed_streams(emu, files, level):
    r, bad, rates, _ = _run(emu, files["made"], level)
    assert r.returncode == 0 and bad == 0, r.stdout + r.stderr


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_constructed_cases_occur(emu, files, level):
    """Every constructed stream makes some lane fail validation where it was built to: a dead winner or a dead long
    step, behind the opening group or inside it."""
    def fails(name):
        r, bad, rates, lanes = _run(emu, files[name], level)
        assert bad == 0, r.stdout
        return rates, lanes
    rates, (dead, lng) = fails("foreign-long")  # 7-bit form: the neighbouring bucket's members match the whole signature
    assert lng > 0 and rates["failed"] > 0 and rates["ofailed"] > 0
    rates, (dead, lng) = fails("foreign-short")
    assert dead > 0 and lng == 0 and rates["failed"] > 0 and rates["ofailed"] > 0
    for hi in ("", "+hi"):  # an occurrence too far back is dead in either form
        rates, (dead, lng) = fails("window-late" + hi)
        assert lng > 0 and rates["failed"] > 0
        rates, (dead, lng) = fails("window-early" + hi)
        assert lng > 0 and rates["ofailed"] > 0
        rates, (dead, lng) = fails("head-edge" + hi)
        assert lng > 0 and rates["ofailed"] > 0
    rates, (dead, lng) = fails("ramp")
    assert lng >= 64 and rates["failed"] > 0
    rates, _ = fails("ramp-plain")
    assert rates["ends"] > 0


def test_model_reports_a_dead_winner_that_is_kept(emu, files):
    """The check can fail: without the look at the winner's key a dead step's match replaces the lane's best."""
    r, bad, _, _ = _run(emu, files["made"], 6, "break")
    assert r.returncode == 1 and bad > 0, r.stdout + r.stderr


def test_group_rates_on_text(emu, files):
    """The rates the kernel's counters are set against (level 6, T-corpus): about ten groups behind the opening
    group per chunk, four of them with a chain's end, and under a third of those fail validation."""
    r, bad, rates, _ = _run(emu, files["text"], 6)
    assert bad == 0, r.stdout
    assert 4.0 < rates["fast"] < 8.0 and 3.0 < rates["ends"] < 5.0, r.stdout
    assert rates["failed"] < rates["ends"] / 3, r.stdout
