"""The sparse page table's words on the CPU.

numamma_amd/csrc/nmg_internal.h holds the host side of the compacted (key,
value) words every reader of the sparse page table downloads: their sort by key
(nmg_sparse_export), the merge of equal keys with a u32 sum (the multi-GPU
merge) and their placement as (entry, thread, page, value) rows (the page-cell
and cost-cell getters, the results snapshot); it needs no HIP and no engine.
tests/c/nmg_sparse_words_host.cpp drives them through no word, one word, two
sparse entries with interleaved words, every kind of word that is skipped, u32
and u64 rows, and three concatenated parts with shared keys and a wrapping sum,
each result against a direct restatement; compiled with g++ as
tests/test_layout_host.py compiles its programs: under the address and
undefined-behaviour sanitizers where the compiler has them, linked statically.
"""
from test_layout_host import SAN, _build_and_run


def test_sparse_words(tmp_path):
    out, err = _build_and_run("nmg_sparse_words_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_sparse_words_host", str(tmp_path))
    assert out is not None, err
