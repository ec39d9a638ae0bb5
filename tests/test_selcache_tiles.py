"""The second trips of the selector-cache kernels' loops, on the CPU: every
case of selcache_tiles_util.py through the library's host walkers
(diag_cpu=True) on a host-only handle, so each input and each oracle is
validated without a GPU.  Device-dependent shapes are built for 256 CUs.  The
same checks run through the kernels in test_selcache_tiles_gpu.py."""
import pytest

import selcache_tiles_util as T
import selcache_util as U


@pytest.fixture()
def sc(host):
    s = host.selector_cache()
    yield s
    s.destroy()


@pytest.mark.parametrize("n_rules", T.TILE_RULES)
def test_reach_rule_tiles(sc, n_rules):
    T.check_reach_tiles(sc, n_rules, diag_cpu=True)


def test_reach_wider_than_one_block(sc):
    T.check_reach_wide(sc, diag_cpu=True)


def test_match_wider_than_one_block_chunk_32(sc):
    assert T.wide_match_selectors(T.CPU_CUS) == 1925
    T.check_match_wide(sc, T.CPU_CUS, diag_cpu=True)


def test_reach_more_endpoints_than_one_launch(sc):
    T.check_reach_many_endpoints(sc, diag_cpu=True)


def test_empty_identity_table(sc):
    T.check_empty_table(sc, diag_cpu=True)
    U.check_match(sc, 65, diag_cpu=True)


def test_match_long_identities_values_requirements(sc):
    T.check_match_long(sc, diag_cpu=True)


def test_expand_more_rows_than_chunk_and_grids(sc):
    T.check_expand_many_rows(sc, T.CPU_CUS, diag_cpu=True)


def test_expand_wide_rows_grid_stride(sc):
    T.check_expand_wide_rows(sc, T.CPU_CUS, diag_cpu=True)


def test_fused_entries_more_rows_than_count_grid(sc):
    T.check_fused_many_rows(sc, T.CPU_CUS, diag_cpu=True)
