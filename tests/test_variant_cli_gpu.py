"""`mhap-hip --realign --variant-filter` on the error-free planted diploid (tests/variant_cases.py) against the two Python tools run on
the driver's own stdout: the site table equals `python -m mhap_amd.variants --table`, the layout equals `python -m mhap_amd.graph
--variant-filter`, with the repeat filter and the trimming behind it too (the second pass feeds all three stages), the switch takes
cross-haplotype links out of the graph, and without it the driver says nothing of the stage."""
import os
import subprocess
import sys

import pytest

import variant_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
pytestmark = pytest.mark.gpu

P = dict(min_depth=4, min_minor=2, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # six reads deep at the most
VARIANT = [x for k, v in P.items() for x in (f"--variant-{k.replace('_', '-')}", str(v))]
SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]
SCALED_PY = ["--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300"]
TRIM = ["--trim", "--trim-end-clip", "100", "--trim-min-span", "500"]


def driver(directory, fasta, flags):
    os.makedirs(directory)
    r = subprocess.run([CLI, "-s", fasta, "--realign"] + flags, capture_output=True, text=True, timeout=600, cwd=directory)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(os.path.join(directory, "overlaps.txt"), "w") as fh:
        fh.write(r.stdout)
    return r


def tool(module, args):
    r = subprocess.run([sys.executable, "-m", module] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def links(gfa):
    return [tuple(int(x) for x in (f[1], f[3])) for f in (l.split("\t") for l in gfa.decode().split("\n")) if f[0] == "L"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("variant_cli")
    d = vc.planted_diploid()
    fasta = str(tmp / "reads.fasta")
    with open(fasta, "w") as fh:
        for i, r in enumerate(d["reads"]):
            fh.write(f">read{i}\n{r.decode()}\n")
    out = dict(d=d, fasta=fasta, tmp=tmp)
    out["plain"] = driver(str(tmp / "plain"), fasta, ["--gfa", "layout.gfa"] + SCALED)
    out["variant"] = driver(str(tmp / "variant"), fasta, ["--variant-filter", "--variant-table", "sites.tsv", "--gfa", "layout.gfa"] + VARIANT + SCALED)
    out["all"] = driver(str(tmp / "all"), fasta, ["--variant-filter", "--repeat-filter", "--gfa", "layout.gfa"] + VARIANT + TRIM + SCALED)
    return out


def test_stdout_is_unchanged_and_the_stage_speaks_only_when_asked(runs):
    lines = {k: sorted(runs[k].stdout.split("\n")) for k in ("plain", "variant", "all")}   # (the search prints its overlaps in no fixed order)
    assert lines["variant"] == lines["plain"] == lines["all"] and len(lines["plain"]) > 100
    assert "--variant" not in runs["plain"].stderr and "Variant sites" not in runs["plain"].stderr and "variant sites" not in runs["plain"].stderr
    said = runs["variant"].stderr.split("\n")
    assert sum(l.startswith("Variant sites: 30 reads, ") for l in said) == 1
    assert sum(l.startswith("Time (s) to mark variant sites and judge: ") for l in said) == 1
    prefixes = ("Time (s) to realign", "Variant sites:", "Repeats:", "Trim:", "String graph")   # the filter finishes in front of the stages it feeds
    assert [p for l in runs["all"].stderr.split("\n") for p in prefixes if l.startswith(p)] == list(prefixes)


def test_the_table_and_the_layout_equal_the_tools(runs):
    tmp, fasta = runs["tmp"], runs["fasta"]
    overlaps = str(tmp / "variant" / "overlaps.txt")
    py = [x.replace("--variant-", "--") for x in VARIANT]
    t = tool("mhap_amd.variants", [overlaps, fasta, "--table", str(tmp / "py_sites.tsv"), "--judged", str(tmp / "py_judged.tsv"), "-o", str(tmp / "py_kept.txt")] + py)
    assert read(tmp / "py_sites.tsv") == read(tmp / "variant" / "sites.tsv") and len(read(tmp / "py_sites.tsv")) > 0
    said = [l for l in runs["variant"].stderr.split("\n") if l.startswith("Variant sites:")]
    assert [l for l in t.stderr.split("\n") if l.startswith("Variant sites:")] == said
    tool("mhap_amd.graph", [overlaps, fasta, "--variant-filter", "-o", str(tmp / "py_layout.gfa")] + VARIANT + SCALED_PY)
    assert read(tmp / "py_layout.gfa") == read(tmp / "variant" / "layout.gfa")
    tool("mhap_amd.graph", [overlaps, fasta, "--variant-filter", "--repeat-filter", "-o", str(tmp / "py_all.gfa")] + VARIANT + TRIM + SCALED_PY)
    assert read(tmp / "py_all.gfa") == read(tmp / "all" / "layout.gfa")


def test_cross_haplotype_links_leave_the_graph(runs):
    d = runs["d"]
    place, planted = d["place"], d["planted"]
    with_, without = links(read(runs["tmp"] / "variant" / "layout.gfa")), links(read(runs["tmp"] / "plain" / "layout.gfa"))
    first = min(min(l) for l in without)
    assert first in (0, 1)                                                       # the ids are the reads' places in the file
    cross = lambda ls: [(x - first, y - first) for x, y in ls if place[x - first][0] != place[y - first][0]]   # noqa: E731
    assert len(cross(with_)) < len(cross(without))
    listed = {}
    for line in read(runs["tmp"] / "variant" / "sites.tsv").decode().split("\n"):
        if line:
            f = line.split("\t")
            listed.setdefault(int(f[0]) - first, set()).add(vc.genome_position(place, int(f[0]) - first, int(f[1])))
    assert all(g in planted for s in listed.values() for g in s)
    for x, y in cross(with_):                                                    # what stays spans fewer than min_diff listed sites
        lo, hi = max(place[x][1], place[y][1]), min(place[x][2], place[y][2])
        n = sum(lo <= g < hi and (g in listed.get(x, ()) or g in listed.get(y, ())) for g in planted)
        assert n < P["min_diff"], (x, y, n)
