"""The chunk pool's layout rule on the CPU.

numamma_amd/csrc/nmg_pool_layout.h places the route pass's per-workgroup chunk
ranges in a pool of 2^K-chunk pieces; it needs no HIP.  tests/c/
nmg_pool_layout_host.cpp drives it through hand-made and random capacities
(no range crosses a piece, ranges ascending and disjoint and at least their
capacity, the id limit, the piece count), compiled with g++ as
tests/test_layout_host.py compiles its programs: under the address and
undefined-behaviour sanitizers where the compiler has them, linked statically.
"""
from test_layout_host import SAN, _build_and_run


def test_pool_layout(tmp_path):
    out, err = _build_and_run("nmg_pool_layout_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_pool_layout_host", str(tmp_path))
    assert out is not None, err
