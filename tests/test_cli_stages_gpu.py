"""The driver's stages behind --realign, run together: by the flags' own help text the printed overlaps, --correct and --realign-paf stay
on all overlaps, --gfa and --trim do not see --best-overlaps, and --correct sees neither --trim nor --repeat-filter.  So a run with every
stage writes, file for file and line for line, what the runs with a part of the stages write.  The other driver tests run each stage
mostly alone; this one pins which stage feeds which."""
import os
import re
import subprocess

import numpy as np
import pytest

import mhap_amd
from mhap_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
pytestmark = pytest.mark.gpu

SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]            # (as test_trim_gpu.py scales them to these reads)
TRIM = ["--trim", "--trim-end-clip", "100", "--trim-min-span", "500", "--trim-fasta", "t.fa", "--trim-table", "t.tsv"]
SELECT_CORRECT = ["--correct", "c.fa", "--best-overlaps", "2", "--best-min-span", "100", "--best-table", "b.tsv"]
REPEAT_GRAPH = ["--gfa", "g", "--gfa-unitigs", "u", "--gfa-clean", "--gfa-consensus", "--gfa-consensus-fasta", "k.fa", "--repeat-filter", "--repeat-table", "r.tsv"] + SCALED
RUNS = {
    "A": SELECT_CORRECT,
    "B": REPEAT_GRAPH + TRIM,
    "C": SELECT_CORRECT + REPEAT_GRAPH + TRIM,
    "D": SELECT_CORRECT + REPEAT_GRAPH + TRIM + ["--realign-paf"],
    "E": ["--realign-paf"],
    "F": REPEAT_GRAPH + SELECT_CORRECT,      # no --trim: the graph takes the repeat stage's survivors as realigned, and the consensus with them
    "G": REPEAT_GRAPH,
}
STAGE_LINES = ("Best overlaps:", "Corrected", "Repeats:", "Trim:", "String graph", "Cleaned", "Unitigs:", "Consensus:")   # in the order the stages finish


class Run:
    def __init__(self, directory, fasta, flags):
        os.makedirs(directory)
        r = subprocess.run([CLI, "-s", fasta, "--realign"] + flags, capture_output=True, text=True, timeout=600, cwd=directory)
        assert r.returncode == 0, r.stderr[-2000:]
        self.lines = sorted(l for l in r.stdout.split("\n") if l)
        self.stderr = r.stderr.split("\n")
        self.stages = [l for l in self.stderr if l.startswith(STAGE_LINES)]
        self.files = {}
        for name in sorted(os.listdir(directory)):
            with open(os.path.join(directory, name), "rb") as fh:
                self.files[name] = fh.read()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Reads of 2 500 - 3 500 bases at 10 % error, about 25 x over a drawn circular genome of 20 kb, 12 of them made chimeric, as
    test_trim_gpu.py's E2E draws them; the genome carries three copies of a 1.5-kb stretch, so that the repeat stage marks intervals
    (without them it sets overlaps aside and its table stays empty)."""
    tmp = tmp_path_factory.mktemp("cli_stages")
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 4, 20000).astype(np.uint8)
    for c in (9000, 15000):
        codes[c:c + 1500] = codes[2000:3500]
    plain = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 170).astype(np.int32), seed=9, error_rate=0.10)
    fa, _ = workloads.plant_chimeras(plain, 12, seed=5)
    fasta = str(tmp / "reads.fasta")
    with open(fasta, "w") as fh:
        for i in range(len(fa)):
            fh.write(f">read{i}\n{fa.sequence(i)}\n")
    return {name: Run(str(tmp / name), fasta, flags) for name, flags in RUNS.items()}


def _stage(run, prefix):
    return [l for l in run.stages if l.startswith(prefix)]


def test_every_stage_together_writes_what_the_stages_write_apart(runs):
    a, b, c = runs["A"], runs["B"], runs["C"]
    assert set(a.files) == {"c.fa", "b.tsv"} and set(b.files) == {"g", "u", "k.fa", "r.tsv", "t.fa", "t.tsv"}
    assert set(c.files) == set(a.files) | set(b.files)
    for name, data in c.files.items():
        assert data == (a.files if name in a.files else b.files)[name], name
    assert c.lines == a.lines == b.lines and len(c.lines) > 1000
    assert c.stages == a.stages + b.stages
    assert [l.startswith(p) for l, p in zip(c.stages, STAGE_LINES)] == [True] * len(STAGE_LINES) and len(c.stages) == len(STAGE_LINES)


def test_paf_output_changes_no_stage(runs):
    a, b, c, d, e = (runs[k] for k in "ABCDE")
    assert d.files == c.files and d.stages == c.stages
    assert d.lines == e.lines and len(d.lines) == len(c.lines) and d.lines != c.lines
    assert all("\tcg:Z:" in l for l in d.lines) and not e.files and not e.stages


def test_graph_on_the_repeat_survivors_as_realigned(runs):
    """Without --trim the graph and its consensus take the repeat stage's survivors as they were realigned, not cut; the selection and
    the correction beside them change neither."""
    a, b, f, g = (runs[k] for k in "ABFG")
    assert set(g.files) == {"g", "u", "k.fa", "r.tsv"} and set(f.files) == set(g.files) | set(a.files)
    for name, data in f.files.items():
        assert data == (g.files if name in g.files else a.files)[name], name
    assert f.lines == g.lines == a.lines and f.stages == a.stages + g.stages
    assert _stage(g, "Repeats:") == _stage(b, "Repeats:") and g.files["r.tsv"] == b.files["r.tsv"]
    assert g.files["g"] != b.files["g"] and not _stage(g, "Trim:")             # (the trimmed reads give another graph)


def test_every_stage_did_something(runs):
    """A run in which nothing happened must not count as passing."""
    c = runs["C"]
    for name in ("r.tsv", "t.tsv", "b.tsv", "u", "k.fa", "c.fa", "t.fa", "g"):
        assert len(c.files[name]) > 0, name
    aside = [re.search(r"\((\d+) of (\d+) overlaps set aside\)", l) for l in c.stderr if l.startswith("Time (s) to mark repeats:")]
    assert len(aside) == 1 and 0 < int(aside[0].group(1)) < int(aside[0].group(2))
    trim = re.match(r"Trim: (\d+) reads, (\d+) deleted, (\d+) cut at 5', (\d+) cut at 3'", _stage(c, "Trim:")[0])
    assert int(trim.group(1)) == 170 and int(trim.group(3)) + int(trim.group(4)) >= 1
    best = re.match(r"Best overlaps: (\d+) reads, (\d+) with a view, (\d+) cut; (\d+) of (\d+) views kept", _stage(c, "Best overlaps:")[0])
    assert 0 < int(best.group(4)) < int(best.group(5))
    assert b"\nL\t" in c.files["g"] and c.files["u"].count(b"\nS\t") >= 1 and c.files["k.fa"].startswith(b">utg")
