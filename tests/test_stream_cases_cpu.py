"""tests/stream_cases.py against include/vaenmf.h, without a GPU: every entry point that takes a stream has a stream case (or
a stated reason to have none), the EM subset reaches every kernel form the full contract list reaches, and the cases that
are excused from the pending check or from capture are those the header's own text excuses."""
import os
import re

import contract_cases as cc
import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "vaenmf.h")) as f:
        return f.read()


def _stream_prototypes():
    """Names of the prototypes with a `void* stream` parameter, comments stripped."""
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    protos = re.findall(r"\b(vaenmf_\w+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S)
    assert len(protos) > 80, len(protos)
    return sorted(name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args))


def test_every_entry_point_with_a_stream_has_a_case():
    protos = _stream_prototypes()
    assert len(protos) == 50, (len(protos), protos)
    named = {e for c in sc.CASES for e in c.entries}
    assert not named & set(sc.EXCLUDED), named & set(sc.EXCLUDED)
    missing = [p for p in protos if p not in named and p not in sc.EXCLUDED]
    assert not missing, "entry points with a stream parameter and no stream case: %s" % missing
    unknown = sorted((named | set(sc.EXCLUDED)) - set(protos))
    assert not unknown, "named by the case table, not a prototype with a stream parameter: %s" % unknown
    assert sorted(sc.EXCLUDED) == ["vaenmf_hbm_read_probe", "vaenmf_wave_sum_probe"]
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)


def test_a_removed_case_is_noticed():
    """The check above fails when the table loses an entry point (here: without the segment case)."""
    named = {e for c in sc.CASES if c.name != "segments" for e in c.entries}
    assert [p for p in _stream_prototypes() if p not in named and p not in sc.EXCLUDED] == ["vaenmf_blend_rows", "vaenmf_gather_rows"]


def test_em_subset_reaches_every_kernel_form():
    forms = lambda cases: {(k, cc.case_class(c)[k]) for c in cases for k in ("chain_kernel", "w_fused")}
    full = forms(cc.CASES)
    sub = forms(cc.BY_NAME[n] for n in sc.EM_SUBSET)
    assert sub == full, sorted(full - sub)
    assert {v for k, v in sub if k == "chain_kernel"} == {0, 1, 2, 3} and {v for k, v in sub if k == "w_fused"} == {0, 1, 2}, sorted(sub)
    names = {c.name for c in sc.CASES}
    for n in sc.EM_SUBSET:
        assert "em_stored_" + n in names
        assert cc.is_wide(cc.BY_NAME[n]) or "em_decoding_" + n in names
    assert {"em_run_" + n for n in sc.EM_RUN} <= names


def test_only_the_header_excuses_a_case():
    text = _header()
    for fn, words in sc.SYNCHRONISES.items():
        assert words in text, (fn, words)
        assert text.index(words) < text.index("int %s(" % fn) < text.index(words) + 2500, fn      # the words stand in fn's own comment
    assert sorted(sc.SYNCHRONISES) == ["vaenmf_bind_batch_async", "vaenmf_lorenz_labels"]
    syncing = [c.name for c in sc.CASES if c.syncs]
    assert syncing == ["bind_new_structure_f257", "lorenz_labels"], syncing
    for c in sc.CASES:
        if c.syncs:
            assert set(c.entries) & set(sc.SYNCHRONISES), c.name
        pending = [p for _, p in c.steps]
        if "vaenmf_em_run" in c.entries:
            assert c.steps == sc.EM_RUN_STEPS and pending == [True, False, True]      # the capturing call alone is excused
        else:
            assert pending == [True], c.name
        # capture: every case but the synchronising ones, vaenmf_em_run and vaenmf_bind_batch_async (whose reason the header states)
        excused = c.syncs or "vaenmf_em_run" in c.entries or "vaenmf_bind_batch_async" in c.entries
        assert (c.capture is not None) == excused, c.name
    assert "may not be called while a caller's stream capture is open" in text
