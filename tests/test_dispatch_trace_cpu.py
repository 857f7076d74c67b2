"""Which kernel family a shape gets, pinned without a GPU: `make -C dct_pruning_amd/csrc trace` builds api.hip with every
dispatcher redirected to a recorder (tests/native/dispatch_trace.cpp) and runs the driver as a fresh process with the GPU
hidden. The AUTO part of the trace - every edge, pad flag on and off, 16-byte / 4-byte base / pitched rows, energies and
coefficients, the multi-tensor calls - must equal tests/golden/dispatch_trace_auto.txt: a change of the AUTO policy is a
reviewed diff of that file (regenerate it with the same make target)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dct_pruning_amd", "csrc")


def _auto_part(text):
    lines = text.splitlines()
    return lines[lines.index("# AUTO begin"):lines.index("# AUTO end") + 1]


def test_auto_dispatch_matches_golden():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    env = {k: v for k, v in os.environ.items() if k != "DCTS_SPLIT_CHUNK_MB"}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # the make recipe sets these too; the driver refuses to start otherwise
    p = subprocess.run(["make", "-j6", "-C", CSRC, "trace"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=1500, env=env)
    assert p.returncode == 0, p.stdout[-4000:]
    got = _auto_part(open(os.path.join(CSRC, "_obj", "dispatch_trace.txt")).read())
    want = _auto_part(open(os.path.join(ROOT, "tests", "golden", "dispatch_trace_auto.txt")).read())
    assert len(got) > 2000
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, "first differing AUTO line %d:\n  got  %s\n  want %s" % diff[0]
    assert len(got) == len(want)
    # a shape that fell from its kernel to the cosine-matrix fallback would still pass parity: spot-check the trace itself
    assert any(l.startswith("e 72x72 p0 a0 a : tile2g 72 ") for l in got)
    assert any(l.startswith("e 224x224 p0 a0 a : tile2d 224 ") for l in got)
    assert any(l.startswith("e 56x56 p0 a0 a : codelet st0 56x56 ") for l in got)
    assert any(l.startswith("e 67x67 p0 a0 a : direct st0 67x67 p0 ") for l in got)
    # api.hip launches nothing itself: every call is on record to its end
    assert not [l for l in got if l.endswith("launch")]
