"""CPU: tests/golden/deflate_params.json is what C zlib 1.2.11 produces for the cases of
tests/paramcases.py (gen_deflate_params.py --check), every yardstick output inflates back to
its input, and the distance cases are what they say.  Skips when the runtime zlib is another
version: the goldens are 1.2.11's."""
import os
import subprocess
import sys
import zlib

import pytest

import paramcases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="the goldens are zlib 1.2.11's")


def test_goldens_are_zlib_1_2_11():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_deflate_params.py"), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases match" % len(cases.all_cases()) in r.stdout


def test_every_case_has_a_golden_and_the_names_are_unique():
    names = [c[0] for c in cases.all_cases()]
    assert len(set(names)) == len(names) and set(names) == set(cases.golden())


def test_the_distance_cases_are_what_they_say():
    for c in cases.group("dist"):
        found, want = cases.dist_found(c, cases.yardstick(c))
        assert found == want, c[0]


def test_the_filler_has_no_repeated_trigram():
    x = cases.filler(70000)
    assert len({x[i:i + 3] for i in range(len(x) - 2)}) == len(x) - 2
