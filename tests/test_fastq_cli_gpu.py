"""FASTQ input and --weigh-qualities end to end: `mhap-hip -s reads.fastq` without the switch writes what it writes for the FASTA
twin, stage for stage; with the switch the driver's files are those of `python -m mhap_amd.correct` and `python -m mhap_amd.graph`
with theirs; the refusals exit 1 with one line."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
KMERS = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip-kmers")
SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]
TOOL_SCALED = ["--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300"]


def _cli(args, cwd=None, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout, cwd=cwd)


def _tool(module, args):
    return subprocess.run([sys.executable, "-m", module] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)


def _records(stdout):
    """The overlap lines of a run, sorted: the order in which a run prints its batches is not fixed, between two runs of one file either."""
    return sorted(stdout.split(b"\n"))


def _lines(stderr, word):
    text = stderr.decode() if isinstance(stderr, bytes) else stderr
    return [l for l in text.split("\n") if l.startswith(word)]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The layout of tests/test_quality_cli_gpu.py's consensus test (170 reads of 2 500 - 3 500 bases at 10 % error over 20 kb) as a
    FASTQ file, its sequence and qualities wrapped at 1 000 bytes and a quality drawn per base, its FASTA twin, and the plain search."""
    d = tmp_path_factory.mktemp("fastq_cli")
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 4, 20000).astype(np.uint8)
    fa = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 170).astype(np.int32), seed=9, error_rate=0.10)
    fastq, twin = str(d / "reads.fastq"), str(d / "twin.fasta")
    with open(fastq, "w") as fq, open(twin, "w") as ft:
        for i in range(len(fa)):
            seq = fa.sequence(i)
            q = "".join(chr(33 + int(x)) for x in rng.choice([3, 5, 9, 14, 22, 31, 40], len(seq)))
            q = "@" + q[1:] if i % 2 else q                              # every other record's qualities open with '@'
            wrap = lambda s: "\n".join(s[k:k + 1000] for k in range(0, len(s), 1000))   # noqa: E731
            fq.write(f"@read{i} extra\n{wrap(seq)}\n+\n{wrap(q)}\n")
            ft.write(f">read{i} extra\n{seq}\n")
    plain = _cli(["-s", fastq])
    assert plain.returncode == 0, plain.stderr[-2000:]
    (d / "ovl.txt").write_bytes(plain.stdout)
    return d, fastq, twin, plain


def _stages(d, tag, reads, extra=()):
    names = {k: str(d / f"{tag}.{k}") for k in ("c.fa", "c.fq", "gfa", "utg.gfa", "k.fa", "k.fq")}
    run = _cli(["-s", reads, "--realign", "--correct", names["c.fa"], "--correct-fastq", names["c.fq"], "--gfa", names["gfa"], "--gfa-unitigs",
                names["utg.gfa"], "--gfa-consensus", "--gfa-consensus-fasta", names["k.fa"], "--gfa-consensus-fastq", names["k.fq"]] + SCALED + list(extra))
    assert run.returncode == 0, run.stderr[-2000:]
    return run, {k: open(v, "rb").read() for k, v in names.items()}


def test_fastq_without_the_switch_is_its_fasta_twin(data):
    d, fastq, twin, plain = data
    t = _cli(["-s", twin])
    assert t.returncode == 0 and _records(t.stdout) == _records(plain.stdout) and len(plain.stdout) > 10000
    (rq, fq), (rt, ft) = _stages(d, "q", fastq), _stages(d, "t", twin)
    assert _records(rq.stdout) == _records(rt.stdout) and fq == ft and all(len(v) > 100 for v in fq.values())
    assert b"Weights" not in rq.stderr and b"--weigh" not in rq.stderr
    # the k-mer tool reads FASTQ through the same scan (and, with --hpc, through the whole-file reader)
    for tag, args in (("scan", ["-k", "12"]), ("hpc", ["-k", "12", "--hpc"])):
        outs = []
        for name, reads in (("q", fastq), ("t", twin)):
            o = str(d / f"kmers.{tag}.{name}")
            k = subprocess.run([KMERS, "-o", o] + args + [reads], capture_output=True, timeout=120)
            assert k.returncode == 0, k.stderr[-1000:]
            outs.append(open(o, "rb").read())
        assert outs[0] == outs[1] and len(outs[0]) > 0


def test_weighted_driver_equals_the_tools(data):
    d, fastq, twin, plain = data
    rw, fw = _stages(d, "w", fastq, ["--weigh-qualities"])
    ru, fu = _stages(d, "u", fastq)
    assert fw["c.fa"] != fu["c.fa"] and fw["gfa"] == fu["gfa"] and fw["k.fa"] != fu["k.fa"]    # the graph does not read qualities
    assert b"--weigh-qualities = true" in rw.stderr and b"--weight-q-lo = 7" in rw.stderr and b"--weight-q-hi = 20" in rw.stderr
    line = _lines(rw.stderr, "Weights: ")
    assert len(line) == 1 and line[0].startswith("Weights: q_lo = 7, q_hi = 20; ")
    ovl = str(d / "ovl.txt")
    tc, tq = str(d / "tool.c.fa"), str(d / "tool.c.fq")
    p = _tool("mhap_amd.correct", [ovl, fastq, "-o", tc, "--fastq", tq, "--weigh-qualities"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(tc, "rb").read() == fw["c.fa"] and open(tq, "rb").read() == fw["c.fq"] and _lines(p.stderr, "Weights: ") == line
    tg, tu, tk, tkq = (str(d / n) for n in ("tool.gfa", "tool.utg.gfa", "tool.k.fa", "tool.k.fq"))
    p = _tool("mhap_amd.graph", [ovl, fastq, "-o", tg, "--unitigs", tu, "--consensus", "--consensus-fasta", tk, "--consensus-fastq", tkq,
                                  "--weigh-qualities"] + TOOL_SCALED)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(tu, "rb").read() == fw["utg.gfa"] and open(tk, "rb").read() == fw["k.fa"] and open(tkq, "rb").read() == fw["k.fq"]
    assert _lines(p.stderr, "Weights: ") == line
    # other thresholds through both
    c2, t2 = str(d / "w2.c.fa"), str(d / "tool2.c.fa")
    r2 = _cli(["-s", fastq, "--realign", "--correct", c2, "--weigh-qualities", "--weight-q-lo", "10", "--weight-q-hi", "30"])
    p = _tool("mhap_amd.correct", [ovl, fastq, "-o", t2, "--weigh-qualities", "--weight-q-lo", "10", "--weight-q-hi", "30"])
    assert r2.returncode == 0 and p.returncode == 0, (r2.stderr[-1000:], p.stderr[-1000:])
    assert open(c2, "rb").read() == open(t2, "rb").read() != fw["c.fa"]


@pytest.mark.parametrize("flags,word,on_twin", [
    (["--realign", "--correct", "c.fa", "--weigh-qualities"], "is FASTA", True),
    (["--realign", "--weigh-qualities"], "--correct or --gfa-consensus", False),
    (["--realign", "--correct", "c.fa", "--weight-q-lo", "5"], "--weigh-qualities too", False),
    (["--realign", "--correct", "c.fa", "--weigh-qualities", "--weight-q-lo", "21"], "0 <= --weight-q-lo <= --weight-q-hi <= 93", False),
    (["--realign", "--correct", "c.fa", "--weigh-qualities", "--weight-q-hi", "94"], "0 <= --weight-q-lo <= --weight-q-hi <= 93", False)])
def test_driver_refusals(data, tmp_path, flags, word, on_twin):
    d, fastq, twin, _ = data
    p = _cli(["-s", twin if on_twin else fastq] + flags, cwd=tmp_path, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and word in out, (out, p.stderr[-500:])
    assert not (tmp_path / "c.fa").exists()


def test_tool_refusals(data):
    d, fastq, twin, _ = data
    ovl = str(d / "ovl.txt")
    p = _tool("mhap_amd.correct", [ovl, twin, "--weigh-qualities"])
    assert p.returncode == 1 and p.stdout.count("\n") == 1 and "is FASTA" in p.stdout
    p = _tool("mhap_amd.graph", [ovl, fastq, "--weigh-qualities"])
    assert p.returncode == 1 and p.stdout.count("\n") == 1 and "--consensus too" in p.stdout
    p = _tool("mhap_amd.correct", [ovl, fastq, "--weight-q-hi", "30"])
    assert p.returncode == 2 and "--weigh-qualities" in p.stderr
    p = _tool("mhap_amd.correct", [ovl, fastq, "--weigh-qualities", "--weight-q-lo", "40"])
    assert p.returncode == 2 and "0 <= --weight-q-lo" in p.stderr


def test_a_broken_fastq_is_refused_by_the_driver(tmp_path):
    bad = tmp_path / "bad.fastq"
    bad.write_text("@a\nACGT\n+\nIII\n")
    p = _cli(["-s", str(bad)], timeout=120)
    assert p.returncode != 0 and b"FASTQ record 1 is cut short" in p.stderr + p.stdout
