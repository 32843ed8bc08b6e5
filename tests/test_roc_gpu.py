"""EstimateROC (mhap_amd.roc) end to end on the GPU: c1-shaped reads with their truth, overlaps from MinHashSearch, the GPU aligner
against the CPU restatement of its contract."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
from mhap_amd import roc, workloads  # noqa: E402
import align_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N, L, SEED = 1000, 5000, workloads.SEED ^ 1


@pytest.fixture(scope="module")
def c1(tmp_path_factory):
    d = tmp_path_factory.mktemp("roc")
    fa = mhap_amd.synth_reads(N, L, seed=SEED)
    truth, G = mhap_amd.synth_truth(N, L, seed=SEED)
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=256, device=0)) as ms:
        ms.add_data(fa)
        lines = mhap_amd.records_to_lines(ms.find_matches())
    ovl = d / "ovl.txt"
    ovl.write_text("".join(x + "\n" for x in lines))
    fasta = d / "reads.fasta"
    workloads.write_fasta(fa, fasta, prefix="")
    m4 = d / "truth.m4"
    workloads.write_truth_m4(m4, truth, G)
    # the rescue case: a few reads moved away from where they came from, so their real overlaps are "not in truth"
    moved = truth.copy()
    seen = np.bincount([int(x.split()[k]) - 1 for x in lines for k in (0, 1)], minlength=N)
    seen[truth["start"] + truth["span"] > G] = 0
    movers = np.argsort(-seen, kind="stable")[:2]                      # the two reads with the most records
    moved["start"][movers] = (moved["start"][movers] + G // 2) % max(1, G - 2 * L)
    m4_moved = d / "truth_moved.m4"
    workloads.write_truth_m4(m4_moved, moved, G)
    return dict(fa=fa, ovl=str(ovl), fasta=str(fasta), m4=str(m4), m4_moved=str(m4_moved), n_lines=len(lines))


@pytest.mark.parametrize("trials", [3000, 0])
def test_gpu_aligner_equals_cpu_aligner(c1, trials):
    gpu = roc.estimate_roc(c1["m4"], c1["ovl"], c1["fasta"], trials=trials, dp=True)
    cpu = roc.estimate_roc(c1["m4"], c1["ovl"], c1["fasta"], trials=trials, dp=True, aligner=align_ref.align_pairs)
    assert c1["n_lines"] > 100
    assert (gpu.tp, gpu.fn, gpu.tn, gpu.fp, gpu.lines) == (cpu.tp, cpu.fn, cpu.tn, cpu.fp, cpu.lines)
    assert gpu.tp > 0 and gpu.ppv > 0.5


def test_dp_rescues_moved_reads(c1):
    off = roc.estimate_roc(c1["m4_moved"], c1["ovl"], c1["fasta"], trials=0, dp=False)
    on = roc.estimate_roc(c1["m4_moved"], c1["ovl"], c1["fasta"], trials=0, dp=True)
    cpu = roc.estimate_roc(c1["m4_moved"], c1["ovl"], c1["fasta"], trials=0, dp=True, aligner=align_ref.align_pairs)
    assert on.dp_pairs > 0
    assert on.ppv > off.ppv
    assert (on.tp, on.fp, on.lines) == (cpu.tp, cpu.fp, cpu.lines)


def test_cli_lines_equal_api(c1):
    p = subprocess.run([sys.executable, "-m", "mhap_amd.roc", c1["m4"], c1["ovl"], c1["fasta"], "2000", "0", "true"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    api = roc.estimate_roc(c1["m4"], c1["ovl"], c1["fasta"], 2000, 0, True)
    assert p.stdout.splitlines() == api.lines and len(api.lines) == 3
    assert "Loading reference...done" in p.stderr
