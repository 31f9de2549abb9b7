"""BGZF ranges by virtual offset through the JavaScript host path (js/test/inflate-bgzf-range.test.mjs):
decompressBatch*(inputs, "gzip", {members: "bgzf", ranges: [[vb, ve], ...]}) with BigInt offsets -- two ranges over
one file through the addon, a range that follows no chain between good ones, the capacity outcome, and the rejection
rules.  The argument checks and bgzfRangeOutLength need no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zlib-streams-ts_amd", "js")
ADDON = os.path.join(JS, "zsnapi.node")
TEST = os.path.join(JS, "test", "inflate-bgzf-range.test.mjs")

need_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON),
                               reason="node or the built addon (make -C zlib-streams-ts_amd/js) is missing")


@need_node
def test_js_module_checks_the_ranges_option_without_a_gpu():
    r = subprocess.run(["node", TEST, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")


@need_node
@pytest.mark.gpu
def test_js_two_ranges_over_one_file():
    r = subprocess.run(["node", TEST], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
