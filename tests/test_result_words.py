"""The tagged result words, their wait and the host walks over them (host only, no GPU).

Every run of the planner ends by reading words `tag << 32 | value` out of mapped or shared host memory
(csrc/result_words.hpp): K2's per-candidate words, the ledger step's, K3's header, the other ranks' regions of
the shared-memory transport.  tools/result_words_check.cpp takes the wait (own and peer words, the stream
fallback, stale tags) and every walk against a naive second implementation, a writer thread playing the device
and the peers over heap blocks of exact size; it exits 2 when a run's random cases missed a listed corner."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "k8s-spot-rescheduler_amd", "bin", "result_words_check")


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(TOOL):
        pytest.skip("bin/result_words_check is not built (make -C k8s-spot-rescheduler_amd tools)")
    return TOOL


@pytest.mark.parametrize("cases,seed", [(1500, 1), (1000, 20261)])
def test_walks_equal_the_naive_walks(tool, cases, seed):
    out = subprocess.run([tool, str(cases), str(seed)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("result_words_check ok: %d lists" % cases), out.stdout


def test_a_vacuous_run_does_not_pass(tool):
    """Too few cases to meet every corner: the tool says so instead of passing."""
    out = subprocess.run([tool, "2", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2, out.stdout + out.stderr
    assert "vacuous" in out.stderr
