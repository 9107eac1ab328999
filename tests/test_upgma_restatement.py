"""The numpy restatement of UPGMA5 (tests/_upgma.py) — what the device kernels are checked against — against the compiled reference's
`-upgma5` itself: byte-equal Newick text for every -linkage on plain, -scaledist, -eadist and -reseek input. The committed fixtures
(tests/golden/upgma_*.json, written by tests/golden/make_upgma_golden.py) hold input and Newick text; where the compiled reference is present it
is also run again on the committed input."""
import json
import os
import subprocess
import tempfile

import pytest

import _upgma as U

HERE = os.path.dirname(os.path.abspath(__file__))
MUSCLE = os.path.join(HERE, "..", "oracle", "_ref", "muscle")
MODES = ("plain", "scaledist", "eadist", "reseek")


def fixture(mode):
    with open(os.path.join(HERE, "golden", "upgma_%s.json" % mode)) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_equals_reference_upgma5(mode):
    if not os.path.exists(MUSCLE):
        pytest.skip("oracle/_ref/muscle is not built here")
    fx = fixture(mode)
    for case in fx["cases"]:
        for linkage in U.LINKAGES:
            with tempfile.TemporaryDirectory() as d:
                with open(os.path.join(d, "in.tsv"), "w") as f:
                    f.write(case["input"])
                subprocess.run([MUSCLE, "-upgma5", "in.tsv", "-output", "out.nwk", "-linkage", linkage, "-quiet"] + fx["flags"], check=True, cwd=d,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
                ref = open(os.path.join(d, "out.nwk")).read()
            assert ref == case["newick"][linkage], "the fixture is stale: tests/golden/make_upgma_golden.py"
            assert U.cmd_upgma5(case["input"], mode, linkage) == ref, (mode, case["n"], linkage)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_equals_committed_newick(mode):
    """the same comparison against the committed text alone: runs everywhere"""
    for case in fixture(mode)["cases"]:
        for linkage in U.LINKAGES:
            assert U.cmd_upgma5(case["input"], mode, linkage) == case["newick"][linkage], (mode, case["n"], linkage)
