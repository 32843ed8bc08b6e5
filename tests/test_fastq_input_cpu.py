"""FASTQ input without a GPU ("FASTQ input" in include/mhap_hip.h): both readers against the FASTA twin of every file and the expected
Phred bytes, the refusals with their one line, and the record pass under the sanitizers as a program of its own."""
import bz2
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mhap_amd import api  # noqa: E402


def phred(s):
    return [ord(c) - 33 for c in s]


# name -> (the FASTQ text, [(header line after '@', sequence as written, quality string)] of its records in order)
CASES = {
    "single_line": ("@r1\nACGTAC\n+\nIIII5I\n@r2 more words\nGGT\n+r2 more words\n!~5\n",
                    [("r1", "ACGTAC", "IIII5I"), ("r2 more words", "GGT", "!~5")]),
    "multi_line": ("@m1\nACG\nTACGT\nA\n+\nII\nIIII55\nI\n@m2,x\nTT\n+\n5\n5\n",
                   [("m1", "ACGTACGTA", "IIIIII55I"), ("m2,x", "TT", "55")]),
    "at_and_plus_open_quality_lines": ("@q1\nACGT\n+\n@III\n@q2\nACGTAC\n+\n+II\n@+I\n@q3\nAC\n+\n@\n+\n",
                                       [("q1", "ACGT", "@III"), ("q2", "ACGTAC", "+II@+I"), ("q3", "AC", "@+")]),
    "crlf": ("@c1\r\nACGT\r\n+\r\nI5I5\r\n@c2\r\nGG\r\nCC\r\n+\r\nII\r\n55\r\n", [("c1", "ACGT", "I5I5"), ("c2", "GGCC", "II55")]),
    "cr_only": ("@o1\rACGT\r+\rI5I5\r@o2\rGG\r+\r!!\r", [("o1", "ACGT", "I5I5"), ("o2", "GG", "!!")]),
    "lower_case_and_n": ("@l1\nacgtn\n+\n55555\n@l2\nAcGt\n+\nIIII\n", [("l1", "acgtn", "55555"), ("l2", "AcGt", "IIII")]),
    "empty_record_between": ("@e1\nACG\n+\nIII\n@none\n\n+\n\n@e2\nTTTT\n+\n5555\n", [("e1", "ACG", "III"), ("none", "", ""), ("e2", "TTTT", "5555")]),
    "empty_record_without_blank_lines": ("@e1\nACG\n+\nIII\n@none\n+\n@e2\nT\n+\n~", [("e1", "ACG", "III"), ("none", "", ""), ("e2", "T", "~")]),
    "no_final_line_end": ("@z\nACGT\n+\n!!!~", [("z", "ACGT", "!!!~")]),
}

# name -> (the text, the refusal's one line)
REFUSALS = {
    "missing_plus": ("@a\nACGT\n+\nIIII\n@b\nACGT\n@c\nAC\n+\nII\n", "FASTQ record 2 has no + line after its sequence."),
    "missing_plus_at_the_end": ("@a\nACGT\n", "FASTQ record 1 has no + line after its sequence."),
    "file_ends_in_qualities": ("@a\nACGT\n+\nIIII\n@b\nACGTAC\n+\nIII\n", "FASTQ record 2 is cut short: the file ends before its qualities are complete."),
    "file_ends_before_qualities": ("@a\nACGT\n+\n", "FASTQ record 1 is cut short: the file ends before its qualities are complete."),
    "quality_line_too_long": ("@a\nACGT\n+\nIIIII\n", "FASTQ record 1 has a quality line that runs past its sequence."),
    "second_quality_line_too_long": ("@a\nAC\nGT\n+\nII\nIII\n", "FASTQ record 1 has a quality line that runs past its sequence."),
    "quality_byte_too_low": ("@a\nACGT\n+\nII I\n", "FASTQ record 1 has a quality byte outside 33 .. 126."),
    "quality_byte_too_high": ("@a\nACGT\n+\nII\x7fI\n", "FASTQ record 1 has a quality byte outside 33 .. 126."),
    "record_without_at": ("@a\nACGT\n+\nIIII\nb\nACGT\n+\nIIII\n", "FASTQ record 2 does not start with @. Invalid format."),
}


def twin_text(records):
    return "".join(f">{h}\n{s}\n" for h, s, _ in records)


def expected(records):
    """(names, sequences, Phred bytes) of the non-empty records."""
    kept = [(h, s, q) for h, s, q in records if s]
    names = [h.replace(",", " ").split()[0] for h, _, _ in kept]
    return names, [s.upper() for _, s, _ in kept], [phred(q) for _, _, q in kept]


def write(tmp_path, name, text, opener=open):
    p = str(tmp_path / name)
    with opener(p, "wb") as fh:
        fh.write(text.encode("latin-1"))
    return p


def check_against_twin(fq_path, fa_path, records, id_offset):
    names, seqs, quals = expected(records)
    fq, fa = api.FastaData.from_file(fq_path, id_offset), api.FastaData.from_file(fa_path, id_offset)
    assert fa.qualities is None and fq.qualities is not None and fq.qualities.dtype == np.uint8
    for field in ("bases", "offsets", "lengths", "ids"):
        assert np.array_equal(getattr(fq, field), getattr(fa, field)), field
    assert [fq.sequence(i) for i in range(len(fq))] == seqs
    assert fq.ids.tolist() == [id_offset + 1 + i for i in range(len(seqs))]
    assert fq.qualities.tolist() == [q for per_read in quals for q in per_read]
    with api.FastaScan(fq_path, id_offset) as sq, api.FastaScan(fa_path, id_offset) as sa:
        assert sq.has_qualities and not sa.has_qualities
        (ids_q, lens_q, names_q), (ids_a, lens_a, names_a) = sq.info(), sa.info()
        assert ids_q.tolist() == ids_a.tolist() == fq.ids.tolist() and lens_q.tolist() == lens_a.tolist() == fq.lengths.tolist()
        assert names_q == names_a == names
        assert sq.total_bases == sa.total_bases == len(fq.bases)
        assert np.array_equal(sq.qualities(), fq.qualities)          # mhap_fasta_read and the scan agree
        with pytest.raises(api.MhapError):
            sa.qualities()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("id_offset", [0, 40])
def test_fastq_equals_its_fasta_twin(tmp_path, name, id_offset):
    text, records = CASES[name]
    check_against_twin(write(tmp_path, "reads.fastq", text), write(tmp_path, "twin.fasta", twin_text(records)), records, id_offset)


@pytest.mark.parametrize("suffix,opener", [(".fq.gz", gzip.open), (".fastq.bz2", bz2.open), (".fq", open)])
def test_compressed_and_fq_names(tmp_path, suffix, opener):
    text, records = CASES["multi_line"]
    check_against_twin(write(tmp_path, "reads" + suffix, text, opener), write(tmp_path, "twin.fasta", twin_text(records)), records, 0)


def test_many_records_do_not_depend_on_the_threads(tmp_path):
    """More records than host threads, lengths that vary, qualities that begin with '@': every read's bytes and qualities are its own."""
    rng = np.random.default_rng(3)
    records = []
    for r in range(300):
        n = int(rng.integers(1, 90))
        seq = "".join(rng.choice(list("ACGT"), n).tolist())
        q = "@" + "".join(chr(33 + int(x)) for x in rng.integers(0, 94, n - 1))
        records.append((f"read{r}", seq, q))
    text = "".join(f"@{h}\n{s}\n+\n{q}\n" for h, s, q in records)
    check_against_twin(write(tmp_path, "many.fastq", text), write(tmp_path, "twin.fasta", twin_text(records)), records, 0)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(tmp_path, name):
    text, line = REFUSALS[name]
    p = write(tmp_path, "bad.fastq", text)
    with pytest.raises(api.MhapError) as e:
        api.FastaData.from_file(p)
    assert str(e.value) == line
    with pytest.raises(api.MhapError) as e:
        api.FastaScan(p)
    assert str(e.value) == line


def test_fasta_and_other_first_bytes_are_unchanged(tmp_path):
    p = write(tmp_path, "x.fasta", "ACGT\n")
    for reader in (api.FastaData.from_file, api.FastaScan):
        with pytest.raises(api.MhapError) as e:
            reader(p)
        assert str(e.value) == "Next sequence does not start with >. Invalid format."
    fa = api.FastaData.from_file(write(tmp_path, "y.fastq", ">a\nAC@GT\n>b\n@CG\n"))      # '>' first: FASTA, whatever the name
    assert fa.qualities is None and [fa.sequence(i) for i in range(2)] == ["AC@GT", "@CG"]
    with pytest.raises(api.MhapError):
        api.all_qualities(fa)


def test_the_record_pass_under_the_sanitizers(tmp_path):
    """tools/fastq_host_check.cpp, built with -fsanitize=address,undefined as its first lines say, over every file above and every
    truncation of each: the same record counts and quality sums, the same refusals, and no report from a sanitizer."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fastq_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "fastq_host_check.cpp"), os.path.join(ROOT, "mhap_amd", "csrc", "fastq_host.cpp"), "-o", exe],
                   check=True, cwd=ROOT)
    paths, want = [], []
    for name in sorted(CASES):
        text, records = CASES[name]
        p = write(tmp_path, name + ".fastq", text)
        paths.append(p)
        want.append(f"{p}: {len(records)} records, {sum(len(s) for _, s, _ in records)} bases, quality sum {sum(sum(phred(q)) for _, _, q in records)}")
    for name in sorted(REFUSALS):
        p = write(tmp_path, name + ".fastq", REFUSALS[name][0])
        paths.append(p)
        want.append(f"{p}: refused: {REFUSALS[name][1]}")
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == want + ["fastq_host_check: ok"] and run.stderr == ""
