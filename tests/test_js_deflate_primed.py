"""Primed pieces through the JavaScript host path (js/test/deflate-primed.test.mjs):
compressBatch*(inputs, format, {level, flushAt | flushEvery, primed: true}), goldens of
tests/golden/deflate_primed.json, the outputs read back as one stream through node's zlib and the
engine's inflate, and the rejection rules.  The argument checks need no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zlib-streams-ts_amd", "js")
ADDON = os.path.join(JS, "zsnapi.node")
TEST = os.path.join(JS, "test", "deflate-primed.test.mjs")

need_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON),
                               reason="node or the built addon (make -C zlib-streams-ts_amd/js) is missing")


@need_node
def test_js_module_checks_the_primed_option_without_a_gpu():
    r = subprocess.run(["node", TEST, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")


@need_node
@pytest.mark.gpu
def test_js_compress_primed():
    r = subprocess.run(["node", TEST], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
