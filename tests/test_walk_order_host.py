"""The report's walk order on the CPU.

numamma_amd/csrc/nmg_walk_order.h permutes what the call-site registry reads
per entry to the report's walk positions, rewrites a row array's entry column
and regroups nmg_report's page rows; it needs no HIP and no engine.  tests/c/
nmg_walk_order_host.cpp drives it through an empty order, one entry, a
reversed and a random order of five with repeated entries in rows of 4 and 5
words, and no row at all, each result against a direct restatement; compiled
with g++ as tests/test_layout_host.py compiles its programs: under the address
and undefined-behaviour sanitizers where the compiler has them, linked
statically.
"""
from test_layout_host import SAN, _build_and_run


def test_walk_order(tmp_path):
    out, err = _build_and_run("nmg_walk_order_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_walk_order_host", str(tmp_path))
    assert out is not None, err
