"""The dispatcher of keds_cross_attn_seq without a GPU: keds_cross_seq_plan_query (csrc/cross_seq_plan.h, the function the call
launches from) against the Python model of the plan in tests/cross_seq_check.py and against the form table of docs/kernels.md row by
row.  The document, the model and the library are three statements that must agree."""
import ctypes
import itertools
import os
import re

import pytest

from keds_amd import _lib
from tests import cross_seq_check as cs
from tests.conftest import ROOT

FIELDS = ("form", "nkt", "nfull", "q_per_wg", "grid", "block", "lds", "chunks")      # keds_cross_seq_last_launch's layout
LK, LQ, BHEADS = (1, 32, 33, 96, 97, 288), (1, 16, 17, 257, 1000), (1, 8, 1024)
E_ARG = -1
ROWS = ("tile, 2 key tiles", "tile, 6 key tiles", "tile, 18 key tiles, every tile masked", "tile, 18 key tiles, 16 unmasked")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def query(lib, B, Lq, Lk, heads):
    """one keds_cross_seq_plan_query call, checked against the model -> dict of FIELDS"""
    info = (ctypes.c_int * 8)()
    _lib.check(lib.keds_cross_seq_plan_query(B, Lq, Lk, heads, info), "keds_cross_seq_plan_query")
    assert list(info) == cs.plan(B, Lq, Lk, heads), (B, Lq, Lk, heads)
    return dict(zip(FIELDS, info))


def _splits(n):
    """(B, heads) with B * heads = n"""
    return {1: ((1, 1),), 8: ((1, 8), (8, 1), (2, 4)), 1024: ((128, 8), (64, 16))}[n]


def test_library_plans_what_the_model_plans(lib):
    n = 0
    for Lk, Lq, bh in itertools.product(LK, LQ, BHEADS):
        for B, heads in _splits(bh):
            got = query(lib, B, Lq, Lk, heads)
            assert got["grid"] == bh * got["chunks"] and got["chunks"] * got["q_per_wg"] >= Lq
            n += 1
    assert n == 6 * 5 * 6


def test_every_key_count_and_the_query_chunks(lib):
    for Lk in range(1, 289):
        for Lq in (1, 288, 289):
            query(lib, 3, Lq, Lk, 2)
    for Lq in (1, 16, 257, 288):                        # up to 288 queries: one workgroup per (sample, head) takes them all
        got = query(lib, 3, Lq, 77, 2)
        assert (got["chunks"], got["q_per_wg"], got["grid"]) == (1, Lq, 6)
    for Lq, chunks in ((289, 2), (512, 2), (513, 3), (1000, 4)):      # beyond: chunks of 256 queries
        got = query(lib, 3, Lq, 77, 2)
        assert (got["chunks"], got["q_per_wg"], got["grid"]) == (chunks, 256, 6 * chunks)


def test_lds_of_the_largest_form_is_two_workgroups_per_cu(lib):
    got = query(lib, 1, 1, 288, 1)
    assert got["lds"] == 74752 and 2 * got["lds"] <= 160 * 1024


# ---- docs/kernels.md: the form table, one test per row ------------------------------------------------------------------------------
def _table():
    text = open(os.path.join(ROOT, "docs", "kernels.md"), encoding="utf-8").read()
    table = text[text.index("| form of the multi-query cross-attention (recorded) | Lk |"):]
    return table[:table.index("\n\n")]


def _row(name):
    """the cells of a row: (Lk range as (lo, hi), key tiles, unmasked tiles, LDS bytes)"""
    for line in _table().splitlines():
        cells = [c.strip() for c in line.strip("|").split("|")]
        if cells[0] == name:
            lo, hi = (int(x) for x in re.findall(r"\d+", cells[1]))
            return (lo, hi), int(cells[2]), int(cells[3]), int(cells[4].replace(",", ""))
    raise KeyError(name)


def test_the_document_has_exactly_these_rows():
    assert tuple(re.findall(r"^\| ([^|]+?) \|", _table(), flags=re.M)[1:]) == ROWS


@pytest.mark.parametrize("name", ROWS)
def test_row(lib, name):
    (lo, hi), nkt, nfull, lds = _row(name)
    for Lk in range(lo, hi + 1):
        for Lq, (B, heads) in itertools.product((1, 257, 1000), ((1, 1), (128, 8))):
            got = query(lib, B, Lq, Lk, heads)
            assert (got["form"], got["nkt"], got["nfull"], got["lds"], got["block"]) == (cs.FORM_TILE, nkt, nfull, lds, 256), (name, Lk, got)


def test_the_rows_cover_every_key_count_once():
    spans = sorted(_row(name)[0] for name in ROWS)
    assert spans[0][0] == 1 and spans[-1][1] == 288
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert lo == hi + 1


# ---- failure behaviour ----------------------------------------------------------------------------------------------------------------
def test_query_with_a_bad_argument_returns_e_arg_and_leaves_info_untouched(lib):
    info = (ctypes.c_int * 8)(*([-5] * 8))
    for B, Lq, Lk, heads in ((3, 1, 0, 2), (3, 1, 289, 2), (3, 1, -1, 2), (0, 1, 77, 2), (3, 0, 77, 2), (3, 1, 77, 0), (-1, 1, 77, 2)):
        assert lib.keds_cross_seq_plan_query(B, Lq, Lk, heads, info) == E_ARG, (B, Lq, Lk, heads)
        assert list(info) == [-5] * 8
    assert "must be in [1,288]" in _lib.last_error() or "bad argument" in _lib.last_error()
    assert lib.keds_cross_seq_plan_query(3, 1, 77, 2, None) == E_ARG
    assert lib.keds_cross_seq_last_launch(None) == E_ARG


def test_no_launch_yet_reads_as_no_form(lib):
    """the record is per thread: a thread that never launched reads form NONE"""
    import threading
    got = []

    def run():
        info = (ctypes.c_int * 8)(*([-5] * 8))
        got.append((lib.keds_cross_seq_last_launch(info), list(info)))

    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert got == [(0, [0] * 8)]
