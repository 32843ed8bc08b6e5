"""What the record sessions refuse, word for word and with the code: the begin, add, apply and copy of TrimSession, RepeatSession,
SelectSession and GraphSession, the adds of ConsensusSession and CorrectSession, every session class's lifetime (a second close, a
`with` block that closes the handle the session made), and the prototypes load_library gives the exported symbols.  The table of
reads is four reads, one of them empty; a refused record is always record 2 of its list, so that its index shows in the message."""
import os
import re

import numpy as np
import pytest

import mhap_amd
from mhap_amd import api

import string_graph_ref as sg
from test_unitig_consensus_gpu import PARAMS as GRAPH_PARAMS, Case, steps, ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

IDS, LENS = [1, 2, 3, 4], [100, 200, 0, 300]
GOOD = [sg.record(1, 2, 0, 49, 100, 10, 59, 200, 0), sg.record(2, 4, 0, 99, 200, 0, 99, 300, 1)]
UNKNOWN = sg.record(1, 9, 0, 49, 100, 10, 59, 200, 0)
WRONG_LENGTH = sg.record(1, 2, 0, 49, 101, 10, 59, 200, 0)
OUTSIDE = sg.record(1, 2, 0, 100, 100, 10, 59, 200, 0)
SAYS = {"unknown": "record 2 names read 9, which is not among the reads (code -1)",
        "length": "record 2 gives read 1 the length 101, the reads say 100 (code -1)",
        "outside": "record 2 aligns 0 .. 100 of read 1, which has 100 bases (code -1)"}
TABLE_LENGTH = "read 1 has a negative length or one above 2^31 - 9 (code -1)"

# class, the C prefix, one bad parameter and what begin says of it, begin's words for a negative length, the count of the added
# records, the code of a call that needs a finish, whether an end outside the read is refused
SESSIONS = [
    (api.TrimSession, "mhap_trim", dict(min_cov=0), "min_cov must be >= 1, end_clip and min_span >= 0 (code -1)", TABLE_LENGTH,
     "eligible_records", -1, True),
    (api.RepeatSession, "mhap_repeat", dict(min_run=0), "factor_pct must be >= 100, max_cov >= 0, min_run >= 1 and min_unique >= 0 (code -1)",
     TABLE_LENGTH, "eligible_records", -1, True),
    (api.SelectSession, "mhap_select", dict(best_n=0), "best_n must be >= 1 and min_span >= 0 (code -1)", TABLE_LENGTH, "eligible_records", -4, True),
    (api.GraphSession, "mhap_graph", dict(fuzz=-1), "max_hang, min_ovlp and fuzz must be >= 0 and int_frac_permille in [0, 1000] (code -1)",
     "read 1 has a negative length (code -1)", "records", -1, False),
]
BY_NAME = pytest.mark.parametrize("cls,prefix,bad_param,param_says,length_says,count,state_code,ranges",
                                  SESSIONS, ids=[s[0].__name__ for s in SESSIONS])


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def batch(*recs):
    return np.concatenate(recs)


def says(call, text):
    """`call` raises MhapError whose whole text is `text`."""
    with pytest.raises(api.MhapError) as e:
        call()
    assert str(e.value) == text


def added(s, count):
    """The count of added records of a finish."""
    out = s.finish()
    return (out[1] if isinstance(out, tuple) else out)[count]


@BY_NAME
def test_begin_refusals(ms, cls, prefix, bad_param, param_says, length_says, count, state_code, ranges):
    says(lambda: cls(IDS, LENS[:3], handle=ms), f"{cls.__name__}: 4 ids and 3 lengths")
    says(lambda: cls(IDS, [100, -1, 0, 300], handle=ms), f"{prefix}_begin: {length_says}")
    says(lambda: cls(IDS, LENS, handle=ms, **bad_param), f"{prefix}_begin: {param_says}")


@BY_NAME
def test_add_and_apply_refusals(ms, cls, prefix, bad_param, param_says, length_says, count, state_code, ranges):
    with cls(IDS, LENS, handle=ms) as s:
        needs_finish = f": no {prefix}_finish has completed (code {state_code})"
        if cls is api.GraphSession:
            says(s.unitigs, "mhap_graph_unitigs" + needs_finish)
        else:
            says(lambda: s.apply(batch(*GOOD)), f"{prefix}_apply" + needs_finish)
        if hasattr(s, "table"):
            says(s.table, f"{prefix}_copy" + needs_finish)
        s.add(batch(*GOOD))
        assert added(s, count) == 2
        for what, bad in (("unknown", UNKNOWN), ("length", WRONG_LENGTH)):
            says(lambda: s.add(batch(*GOOD, bad)), f"{prefix}_add: {SAYS[what]}")
            assert added(s, count) == 2                              # a refused add adds nothing
        if ranges:
            says(lambda: s.add(batch(*GOOD, OUTSIDE)), f"{prefix}_add: {SAYS['outside']}")
            assert added(s, count) == 2
            says(lambda: s.apply(batch(*GOOD, UNKNOWN)), f"{prefix}_apply: {SAYS['unknown']}")
        else:                                                        # the graph has no such rule: the record is taken and classed
            s.add(batch(*GOOD, OUTSIDE))
            assert added(s, count) == 5 and len(s.classes()) == 5


@BY_NAME
def test_a_session_of_no_reads(ms, cls, prefix, bad_param, param_says, length_says, count, state_code, ranges):
    with cls([], [], handle=ms) as s:
        assert added(s, count) == 0
        if cls is api.GraphSession:
            assert s.arcs.shape == (0, 7) and s.contained().shape == (0,)
        elif cls is api.SelectSession:
            assert s.rows.shape == (0, 4)
        else:
            assert s.table()[0].shape == (0, 4)


def two_read_graph():
    c = Case()
    c.chain(ur.draw_bases(1500, 95), steps(2, 500, 1000), [0, 1])
    return c


def test_consensus_add_refusals(ms):
    c = two_read_graph()
    recs = c.records()
    with api.GraphSession(c.ids, c.lengths, handle=ms, **GRAPH_PARAMS) as gs:
        gs.add(recs)
        gs.finish()
        gs.unitigs()
        with api.ConsensusSession(gs, c.fasta()) as cs:
            unknown, longer = recs[:1].copy(), recs[:1].copy()
            unknown["to_id"] = 9
            longer["alen"] += 1
            says(lambda: cs.add(batch(recs[:1], recs[:1], unknown)), f"mhap_consensus_add: {SAYS['unknown']}")
            says(lambda: cs.add(batch(recs[:1], recs[:1], longer)),
                 f"mhap_consensus_add: record 2 gives read {int(recs[0]['from_id'])} the length 1001, the reads say 1000 (code -1)")
            cs.add(recs)
            assert cs.run()["members"] == 2                          # the refused adds left nothing behind


def four_reads():
    bases = np.frombuffer(ur.draw_bases(sum(LENS), 7), np.uint8)
    offsets = np.concatenate([[0], np.cumsum(LENS)])[:4].astype(np.int64)
    return mhap_amd.FastaData(bases, offsets, np.array(LENS, np.int32), np.array(IDS, np.int64))


def test_correct_add_refusals(ms):
    eq = lambda n: (n << 4) | 7                                      # a run of n '=' columns
    with api.CorrectSession(four_reads(), handle=ms) as cs:
        for what, bad in (("unknown", UNKNOWN), ("length", WRONG_LENGTH)):
            says(lambda: cs.add(batch(*GOOD, bad), [0, 1, 2, 3], [eq(50), eq(100), eq(50)]), f"mhap_correct_add: {SAYS[what]}")
        cs.add(batch(*GOOD), [0, 1, 2], [eq(50), eq(100)])
        assert cs.finish(min_cov=1)[2] == 0


def lifetimes(ms):
    """(name, a function that makes the session, with the handle given or its own)."""
    fasta, c = four_reads(), two_read_graph()
    table = [(cls.__name__, lambda own, cls=cls: cls(IDS, LENS, **({} if own else dict(handle=ms)))) for cls in (s[0] for s in SESSIONS)]
    table.append(("CorrectSession", lambda own: api.CorrectSession(fasta, **({} if own else dict(handle=ms)))))
    return table, c


def test_close_twice_and_with_exit(ms):
    table, c = lifetimes(ms)
    for name, make in table:
        s = make(False)
        s.close()
        s.close()                                                    # a no-op
        assert not s._s and ms._h.value is not None, name           # a borrowed handle stays open
        with make(True) as s:
            assert s._s and s._ms._h.value is not None, name
        assert not s._s and s._ms._h.value is None, name            # the handle the session made went with it
    with api.GraphSession(c.ids, c.lengths, handle=ms, **GRAPH_PARAMS) as gs:
        gs.add(c.records())
        gs.finish()
        gs.unitigs()
        with api.ConsensusSession(gs, c.fasta()) as cs:
            assert cs._s
        assert not cs._s and gs._s and ms._h.value is not None       # its handle is the graph session's
        cs.close()
        assert gs.info()[0] == 2
    d = api.KsimDevice(handle=ms)
    d.close()
    d.close()
    assert ms._h.value is not None
    with api.KsimDevice() as d:
        own = d.ms
        assert own._h.value is not None
    assert own._h.value is None


# declarations the expression below cannot take apart: name -> parameter count
IRREGULAR = {}


def test_every_exported_symbol_has_the_headers_prototype():
    lib = api.load_library()
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    declared = {m.group(1): 0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1
                for m in re.finditer(r"\b(mhap_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    declared.update(IRREGULAR)
    assert sorted(set(api.EXPORTED_SYMBOLS) - set(declared)) == []
    wrong = {}
    for name in api.EXPORTED_SYMBOLS:
        argtypes = getattr(lib, name).argtypes
        if argtypes is None or len(argtypes) != declared[name]:
            wrong[name] = (None if argtypes is None else len(argtypes), declared[name])
    assert wrong == {}
