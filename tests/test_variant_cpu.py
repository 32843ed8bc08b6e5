"""The variant-site contract without a GPU: the restatement (tests/variant_ref.py) on hand-computed pile-ups at every edge of the
site rule and of the judgement, the restatement alone on the error-free planted diploid (the truth gate of the GPU test, with the
one diagonal the layout gives for a path), the argument refusals of `python -m mhap_amd.variants` and of the graph tool, and the
table's text."""
import numpy as np
import pytest

import consensus_ref as cr
import handmade_paths as hp
import variant_cases as vc
import variant_ref as vr
from align_ref import rc_bytes
from mhap_amd import api, graph, variants


@pytest.mark.parametrize("name,votes,own,p,site,fields", vc.SITE_CASES, ids=[c[0] for c in vc.SITE_CASES])
def test_site_rule_on_hand_computed_pile_ups(name, votes, own, p, site, fields):
    got = vr.site_of(votes, own, p)
    assert got["site"] is site
    assert {k: got[k] for k in fields} == fields


@pytest.mark.parametrize("name,a,b,site_a,site_b,to_rc,want", vc.CLASS_CASES, ids=[c[0] for c in vc.CLASS_CASES])
def test_class_of_a_column(name, a, b, site_a, site_b, to_rc, want):
    assert vr.class_of(a[0], b[0], site_a, site_b, to_rc) == want


@pytest.mark.parametrize("agree,disagree,p,keep", vc.KEEP_CASES)
def test_keep_rule(agree, disagree, p, keep):
    assert vr.keep_of(agree, disagree, p) is keep


def _piled(to_rc):
    """Read 0 with sites at 2 and 7 (alleles own / alt), judged against a read that carries alt at 2 and own at 7."""
    t = vc.Table(5)
    x = t.read(b"ACGTACGTAC")
    t.pile(x, {2: ord("T"), 7: ord("A")})
    s2 = b"ACTTACGTAC"
    y = t.read(rc_bytes(s2) if to_rc else s2)
    t.record(x, y, s2, 0, 0, hp.cigar("2= 1X 7="), to_rc)
    return t, x, y


@pytest.mark.parametrize("to_rc", [0, 1])
def test_judgement_through_the_restatement(to_rc):
    t, x, y = _piled(to_rc)
    v = vr.Variants(t.reads, t.ids, **vc.SMALL)
    v.add(*t.add())
    counts = v.finish()
    assert counts[0] == len(t.reads) and counts[6] == 0
    own = v.sites[int(v.offsets[x]):int(v.offsets[x + 1])]
    assert own[:, 0].tolist() == [2, 7]                                  # G / T at 2, T / A at 7
    assert own[0, 1:3].tolist() == [2, 3] and own[1, 1:3].tolist() == [3, 0]
    keep, tallies = v.apply(*t.add())
    # the last record: column 2 disagrees (G against T), column 7 agrees (T against T)
    assert tallies[-1].tolist() == [2, 1, 1, 0] and keep[-1] == 1
    strict = vr.Variants(t.reads, t.ids, **dict(vc.SMALL, min_diff=1))
    strict.add(*t.add())
    strict.finish()
    assert strict.apply(*t.add())[0][-1] == 0                            # 1 of 2 is 50 %
    # the rule is symmetric: the same alignment written from read B's side
    rec = t.recs[-1][0]
    swapped = np.zeros(1, cr.RECORD_DTYPE)
    swapped[0] = (rec["to_id"], rec["from_id"], rec["score"], 0.0, rec["b1"], rec["b2"], rec["blen"], rec["a1"], rec["a2"], rec["alen"], rec["to_rc"], 0)
    runs = t.paths[-1][::-1] if to_rc else t.paths[-1]
    assert v.judge(swapped[0], runs) == tuple(tallies[-1].tolist())


@pytest.fixture(scope="module")
def diploid():
    d = vc.planted_diploid()
    recs = vc.layout_records(d)
    return d, recs, vc.diagonal_paths(d, recs)


DIPLOID = dict(min_depth=4, min_minor=2, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # six reads deep at the most


def test_planted_diploid_layout(diploid):
    d, recs, (off, ops) = diploid
    assert len(d["reads"]) == 30 and all(len(r) == 4000 for r in d["reads"]) and len(d["planted"]) == 50
    assert sum(p[3] for p in d["place"]) == 14                           # half of them reverse-complemented
    cross = sum(d["place"][int(r["from_id"]) - 1][0] != d["place"][int(r["to_id"]) - 1][0] for r in recs)
    assert 0 < cross < len(recs)
    assert all((int(ops[int(off[q])]) & 15) == cr.OP_EQ and (int(ops[int(off[q + 1]) - 1]) & 15) == cr.OP_EQ for q in range(len(recs)))


def test_the_restatement_alone_meets_the_truth_gate(diploid):
    d, recs, (off, ops) = diploid
    v = vr.Variants(d["reads"], d["ids"], **DIPLOID)
    v.add(recs, off, ops)
    counts = v.finish()
    keep, tallies = v.apply(recs, off, ops)
    cross, aside = vc.check_truth(d, recs, v.offsets, v.sites, keep, DIPLOID, vr.site_of)
    assert counts[2] > 0 and aside > 0 and (tallies[:, 3] == 0).all()    # error-free: no column is "other"


def _refused(main, argv, capsys, words):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert words in capsys.readouterr().err


@pytest.mark.parametrize("flag,value", [("--min-depth", 0), ("--min-minor", 0), ("--min-diff", 0), ("--min-pct", 101), ("--max-del-pct", -1),
                                        ("--diff-pct", 101)])
def test_the_tool_refuses_parameters_out_of_range(flag, value, capsys):
    _refused(variants.main, ["o.txt", "r.fasta", flag, str(value)], capsys,
             "--min-depth, --min-minor and --min-diff must be >= 1 and --min-pct, --max-del-pct and --diff-pct in 0 .. 100")


def test_the_tool_refuses_a_negative_band(capsys):
    _refused(variants.main, ["o.txt", "r.fasta", "--band", "-1"], capsys, "--band must be >= 0")


def test_the_graph_tool_refuses_variant_parameters_without_the_switch(capsys):
    _refused(graph.main, ["o.txt", "r.fasta", "--variant-min-depth", "5"], capsys, "need --variant-filter")
    _refused(graph.main, ["o.txt", "r.fasta", "--variant-filter", "--variant-diff-pct", "200"], capsys, "--variant-diff-pct in 0 .. 100")


def test_defaults_are_the_headers():
    assert api.VARIANT_DEFAULTS == dict(min_depth=8, min_minor=3, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)
    assert variants.parameters(variants.argparse.Namespace(**api.VARIANT_DEFAULTS))[0] == api.VARIANT_DEFAULTS


def test_format_table():
    ids, offsets = [7, 8, 9], [0, 2, 2, 3]
    sites = np.array([[0, 0, 1, 5, 3, 8], [41, 3, 2, 6, 4, 11], [9, 1, 0, 4, 4, 9]], np.int32)
    assert variants.format_table(ids, offsets, sites) == "7\t0\tA\tC\t5\t3\t8\n7\t41\tT\tG\t6\t4\t11\n9\t9\tC\tA\t4\t4\t9\n"
    assert variants.format_table(ids, [0, 0, 0, 0], np.zeros((0, 6), np.int32)) == ""
    recs = np.zeros(2, api.RECORD_DTYPE)
    recs["from_id"], recs["to_id"] = [1, 2], [2, 3]
    assert variants.format_judged(recs, [[3, 1, 2, 0], [0, 0, 0, 0]], [0, 1]) == "1\t2\t3\t1\t2\t0\t0\n2\t3\t0\t0\t0\t0\t1\n"
    line = api.variant_counts_line([3, 2, 5, 40, 60, 12, 0], 1, 6)
    assert line == "Variant sites: 3 reads, 2 with a site; 5 sites, 40 of 60 positions deep; 12 views, skipped_views = 0; 1 of 6 overlaps set aside"
