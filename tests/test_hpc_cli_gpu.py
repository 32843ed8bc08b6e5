"""The drivers of the homopolymer compression on the GPU: `mhap-hip --hpc` (self, -q, with --realign, refused on .dat),
`mhap-hip-kmers --hpc` and `python -m mhap_amd.hpc`, each against tests/hpc_ref.py and the CPU oracle on the noisy reads of the
motivating figure."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mhap_amd
from mhap_amd import api, hpc, workloads as W

import hpc_cases as hc
import hpc_ref as ref
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
KMERS_CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip-kmers")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def noisy(tmp_path_factory):
    """The 40 noisy reads as a file, their restated compression, and the oracle's records on it carried to raw coordinates."""
    d = tmp_path_factory.mktemp("hpc")
    fa, true = hc.noisy_reads(0.2, seed=20261020)
    path = str(d / "reads.fasta")
    W.write_fasta(fa, path)
    comp = ref.compress(fa)
    oracle = O.run_self(comp["fasta"], nthreads=4)["records"].astype(api.RECORD_DTYPE)
    return dict(dir=d, fasta=fa, path=path, true=true, comp=comp, raw=ref.expand(oracle, comp))


def _lines(text):
    return sorted(l for l in text.split("\n") if l)


def test_self_search_prints_the_expanded_records(noisy):
    r = subprocess.run([CLI, "-s", noisy["path"], "--hpc"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _lines(r.stdout) == sorted(api.records_to_lines(noisy["raw"])) and len(noisy["raw"]) >= len(noisy["true"])
    c = noisy["comp"]["counts"]
    line = api.hpc_counts_line([c[k] for k in api.HPC_COUNTS])
    assert r.stderr.count("Homopolymer compression:") == 1 and line + "\n" in r.stderr
    plain = subprocess.run([CLI, "-s", noisy["path"]], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "Homopolymer" not in plain.stderr and "--hpc" not in plain.stderr
    assert len(hc.pairs_of_lines(_lines(plain.stdout)) & noisy["true"]) * 2 < len(noisy["true"])


def test_query_file_against_the_index(noisy, tmp_path):
    """Reads 1..25 indexed, reads 26..40 as the -q file: the ids of the second file follow the first's."""
    fa = noisy["fasta"]
    a, b = fa.subset(np.arange(25)), fa.subset(np.arange(25, 40))
    W.write_fasta(a, str(tmp_path / "a.fasta"))
    W.write_fasta(b, str(tmp_path / "b.fasta"))
    r = subprocess.run([CLI, "-s", str(tmp_path / "a.fasta"), "-q", str(tmp_path / "b.fasta"), "--hpc", "--no-self"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ra, rb = ref.compress(a), ref.compress(b)
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms:
        ms.add_data(ra["fasta"])
        found = ms.find_matches_stream(rb["fasta"])
    want = ref.expand(found, rb, ra)
    assert _lines(r.stdout) == sorted(api.records_to_lines(want)) and len(want) > 20
    assert set(want["from_id"].tolist()) <= set(range(26, 41)) and set(want["to_id"].tolist()) <= set(range(1, 26))


def test_realign_gets_raw_reads_and_raw_records(noisy):
    r = subprocess.run([CLI, "-s", noisy["path"], "--hpc", "--realign"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _lines(r.stdout)
    assert len(lines) > len(noisy["true"]) // 2
    lengths = noisy["fasta"].lengths
    for l in lines:
        f = l.split()
        assert int(f[7]) == lengths[int(f[0]) - 1] and int(f[11]) == lengths[int(f[1]) - 1], l
        assert 0 <= int(f[5]) < int(f[6]) <= int(f[7]) and 0 <= int(f[9]) < int(f[10]) <= int(f[11]), l


def test_dat_input_is_refused(tmp_path):
    (tmp_path / "reads.dat").write_bytes(b"")
    p = subprocess.run([CLI, "-s", "reads.dat", "--hpc"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and p.stdout.count("\n") == 1 and "--hpc" in p.stdout and ".dat" in p.stdout, (p.stdout, p.stderr[-500:])


def test_kmers_tool_counts_the_compressed_reads(noisy, tmp_path):
    out = tmp_path / "kmers.txt"
    r = subprocess.run([KMERS_CLI, "-o", str(out), "--hpc", "--min-fraction", "0", "-k", "12", noisy["path"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Homopolymer compression:" in r.stderr
    with hpc.compress(noisy["fasta"]) as hp:
        mhap_amd.count_kmers(hp.fasta, k=12, min_fraction=0.0).write(tmp_path / "api.txt")
    assert out.read_bytes() == (tmp_path / "api.txt").read_bytes() and out.stat().st_size > 1000


def test_python_tool_writes_the_restated_reads(noisy, tmp_path):
    out, table = tmp_path / "c.fasta", tmp_path / "map.tsv"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.hpc", noisy["path"], "-o", str(out), "--map", str(table)], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    c, fa = noisy["comp"], noisy["fasta"]
    want = "".join(f">r{i}\n{c['fasta'].sequence(r)}\n" for r, i in enumerate(fa.ids.tolist()))
    assert out.read_text() == want
    rows = [l.split("\t") for l in table.read_text().split("\n") if l]
    assert [(n, int(a), int(b)) for n, a, b, _ in rows] == [(f"r{i}", int(L), int(k)) for i, L, k in zip(fa.ids.tolist(), fa.lengths.tolist(), c["clen"].tolist())]
    assert max(int(m) for *_, m in rows) == c["counts"]["longest_run"]
    assert api.hpc_counts_line([c["counts"][k] for k in api.HPC_COUNTS]) in p.stderr
