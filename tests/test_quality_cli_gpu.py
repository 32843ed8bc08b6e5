"""FASTQ output end to end: `mhap-hip --realign --correct --correct-fastq` and `--gfa-consensus --gfa-consensus-fastq` against
`python -m mhap_amd.correct --fastq` and `python -m mhap_amd.graph --consensus-fastq` on the same overlaps, file for file and line for
line; without the new flags every file is what it was; the new flags without their owners are refused."""
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
GOLD = os.path.join(ROOT, "tests", "golden")
SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]


def _cli(args, cwd=None, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout, cwd=cwd)


def _tool(module, args):
    return subprocess.run([sys.executable, "-m", module] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)


def _quality_lines(stderr):
    text = stderr.decode() if isinstance(stderr, bytes) else stderr
    return [l for l in text.split("\n") if l.startswith("Qualities: ")]


def _fastq_records(text):
    lines = text.split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    recs = [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]
    for name, seq, plus, qual in recs:
        assert name.startswith("@") and plus == "+" and len(seq) == len(qual) and all(33 <= ord(ch) <= 126 for ch in qual)
    return recs


def test_corrected_reads_as_fastq(tmp_path):
    fasta = os.path.join(GOLD, "small_reads.fasta")
    fa0, fa1, fq1, fq2 = (tmp_path / n for n in ("plain.fa", "c.fa", "c.fq", "c2.fq"))
    plain = _cli(["-s", fasta])
    base = _cli(["-s", fasta, "--realign", "--correct", str(fa0)])
    cor = _cli(["-s", fasta, "--realign", "--correct", str(fa1), "--correct-fastq", str(fq1)])
    assert plain.returncode == 0 and base.returncode == 0 and cor.returncode == 0, cor.stderr[-2000:]
    # without the flag nothing of it shows; with it the FASTA file is what it was
    assert b"Qualities" not in base.stderr and b"fastq = " not in base.stderr and b"--quality" not in base.stderr
    assert fa1.read_bytes() == fa0.read_bytes()
    assert b"--correct-fastq = " in cor.stderr and b"--quality-per-vote = 15" in cor.stderr and b"--quality-cap = 60" in cor.stderr
    line = _quality_lines(cor.stderr)
    assert len(line) == 1
    recs = _fastq_records(fq1.read_text())
    fasta_lines = fa1.read_text().split("\n")
    assert [r[0][1:] for r in recs] == [l[1:] for l in fasta_lines[0::2] if l] and [r[1] for r in recs] == fasta_lines[1::2][:len(recs)]
    n_bytes = sum(len(r[1]) for r in recs)
    assert line[0].startswith(f"Qualities: {n_bytes} bytes, ") and len({ch for r in recs for ch in r[3]}) > 3
    # the stand-alone tool on the driver's own plain output
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tfa, tfq = tmp_path / "tool.fa", tmp_path / "tool.fq"
    p = _tool("mhap_amd.correct", [str(tmp_path / "ovl.txt"), fasta, "-o", str(tfa), "--fastq", str(tfq)])
    assert p.returncode == 0, p.stderr[-2000:]
    assert tfa.read_bytes() == fa1.read_bytes() and tfq.read_bytes() == fq1.read_bytes()
    assert _quality_lines(p.stderr) == line
    # other parameters through both
    cor2 = _cli(["-s", fasta, "--realign", "--correct", str(fa1), "--correct-fastq", str(fq2), "--quality-per-vote", "100", "--quality-cap", "93",
                 "--correct-min-coverage", "2"])
    assert cor2.returncode == 0, cor2.stderr[-2000:]
    p = _tool("mhap_amd.correct", [str(tmp_path / "ovl.txt"), fasta, "-o", str(tfa), "--fastq", str(tfq), "--quality-per-vote", "100", "--quality-cap", "93",
                                    "--min-coverage", "2"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert tfq.read_bytes() == fq2.read_bytes() != fq1.read_bytes() and _quality_lines(p.stderr) == _quality_lines(cor2.stderr)


def test_consensus_as_fastq(tmp_path):
    """The layout of tests/test_unitig_consensus_gpu.py's end-to-end test: 170 reads of 2 500 - 3 500 bases at 10 % error over a
    drawn genome of 20 kb."""
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 4, 20000).astype(np.uint8)
    fa = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 170).astype(np.int32), seed=9, error_rate=0.10)
    fasta = str(tmp_path / "reads.fasta")
    with open(fasta, "w") as fh:
        for i in range(len(fa)):
            fh.write(f">read{i}\n{fa.sequence(i)}\n")
    g0, u0, f0, g1, u1, f1, q1 = (tmp_path / n for n in ("a.gfa", "a.utg.gfa", "a.fasta", "b.gfa", "b.utg.gfa", "b.fasta", "b.fastq"))
    plain = _cli(["-s", fasta])
    r0 = _cli(["-s", fasta, "--realign", "--gfa", str(g0), "--gfa-unitigs", str(u0), "--gfa-consensus", "--gfa-consensus-fasta", str(f0)] + SCALED)
    r1 = _cli(["-s", fasta, "--realign", "--gfa", str(g1), "--gfa-unitigs", str(u1), "--gfa-consensus", "--gfa-consensus-fasta", str(f1),
               "--gfa-consensus-fastq", str(q1)] + SCALED)
    assert plain.returncode == 0 and r0.returncode == 0 and r1.returncode == 0, r1.stderr[-2000:]
    assert b"Qualities" not in r0.stderr and b"fastq = " not in r0.stderr and b"--quality" not in r0.stderr
    assert g1.read_bytes() == g0.read_bytes() and u1.read_bytes() == u0.read_bytes() and f1.read_bytes() == f0.read_bytes()
    line = _quality_lines(r1.stderr)
    assert len(line) == 1
    recs = _fastq_records(q1.read_text())
    fasta_lines = f1.read_text().split("\n")
    assert [r[0][1:] for r in recs] == [l[1:] for l in fasta_lines[0::2] if l] and [r[1] for r in recs] == fasta_lines[1::2][:len(recs)]
    assert line[0].startswith(f"Qualities: {sum(len(r[1]) for r in recs)} bytes, ") and len({ch for r in recs for ch in r[3]}) > 3
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tg, tu, tf, tq = (tmp_path / n for n in ("t.gfa", "t.utg.gfa", "t.fasta", "t.fastq"))
    p = _tool("mhap_amd.graph", [str(tmp_path / "ovl.txt"), fasta, "--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300", "-o", str(tg),
                                  "--unitigs", str(tu), "--consensus", "--consensus-fasta", str(tf), "--consensus-fastq", str(tq)])
    assert p.returncode == 0, p.stderr[-2000:]
    assert tu.read_bytes() == u1.read_bytes() and tf.read_bytes() == f1.read_bytes() and tq.read_bytes() == q1.read_bytes()
    assert _quality_lines(p.stderr) == line


@pytest.mark.parametrize("flags,word", [(["--correct-fastq", "c.fq"], "--correct too"),
                                        (["--correct", "c.fa", "--quality-cap", "40"], "--correct-fastq or --gfa-consensus-fastq"),
                                        (["--correct", "c.fa", "--quality-per-vote", "20"], "--correct-fastq or --gfa-consensus-fastq"),
                                        (["--gfa", "g.gfa", "--gfa-unitigs", "u.gfa", "--gfa-consensus-fastq", "k.fq"], "--gfa-consensus too"),
                                        (["--correct", "c.fa", "--correct-fastq", "c.fq", "--quality-per-vote", "0"], "1 to 1000"),
                                        (["--correct", "c.fa", "--correct-fastq", "c.fq", "--quality-cap", "94"], "1 to 93")])
def test_driver_refuses_the_flags_without_their_owners(tmp_path, flags, word):
    p = _cli(["-s", os.path.join(GOLD, "small_reads.fasta"), "--realign"] + flags, cwd=tmp_path, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and word in out, (out, p.stderr[-500:])
    assert not any((tmp_path / n).exists() for n in ("c.fa", "c.fq", "g.gfa", "k.fq"))


def test_driver_lists_the_flags():
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and all(f"\t{n}," in h.stdout for n in ("--correct-fastq", "--gfa-consensus-fastq", "--quality-per-vote", "--quality-cap"))
