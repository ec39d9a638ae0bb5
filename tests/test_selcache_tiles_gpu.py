"""The second trips of the selector-cache kernels' loops, on the GPU: the
checks of test_selcache_tiles.py through selcache_match_kernel,
selcache_reach_kernel and the expansion trio — more than one LDS tile of
rules, more than one block column of words, more than one reach launch, the
label scan past the staged labels, long value sets and requirement lists,
more rows than a scan chunk and than the count and emit grids — plus what
only the device entries reach: endpoint indices outside the identity table
and an empty identity table.  Shapes that depend on the grid sizes are built
from the device's CU count."""
import numpy as np
import pytest

import selcache_expand_util as X
import selcache_tiles_util as T
import selcache_util as U
from cilium_amd.selcache import unpack_rows

pytestmark = [pytest.mark.gpu, pytest.mark.run_last]


@pytest.fixture()
def sc(gpu):
    s = gpu.selector_cache()
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("n_rules", T.TILE_RULES)
def test_gpu_reach_rule_tiles(sc, n_rules):
    T.check_reach_tiles(sc, n_rules, diag_cpu=False)


def test_gpu_reach_wider_than_one_block(sc):
    T.check_reach_wide(sc, diag_cpu=False)


def test_gpu_match_wider_than_one_block_chunk_32(sc, cus):
    T.check_match_wide(sc, cus, diag_cpu=False)


def test_gpu_reach_more_endpoints_than_one_launch(sc):
    T.check_reach_many_endpoints(sc, diag_cpu=False)


def _sentinels(dev, rows, words):
    import torch
    return (torch.full((rows * words,), X.SENTINEL, dtype=torch.int64, device=dev),
            torch.full((rows * words,), X.SENTINEL, dtype=torch.int64, device=dev),
            torch.full((rows,), X.SENTINEL, dtype=torch.uint8, device=dev))


def test_gpu_reach_dev_indices_outside_the_table(sc):
    """An endpoint index >= the identity count yields zero rows and flags 0
    (only the device entry lets one through).  The tables are those of
    U.reach_case(11) cut to its first 130 identities, so that 130 and 131 lie
    outside; a peer's column does not depend on the other peers, so the
    oracle's rows are cut the same way."""
    import torch
    full, repo, (ing_want, eg_want, fl_want) = U.reach_case(11)
    n = 130
    cache = dict(list(full.items())[:n])
    eps = [0, 130, 5, 131, 0xFFFFFFFF, 129]
    inside = [a for a, e in enumerate(eps) if e < n]
    outside = [a for a, e in enumerate(eps) if e >= n]
    assert len(inside) == len(outside) == 3
    assert ing_want[[0, 5, 129], :n].any() and eg_want[[0, 5, 129], :n].any() and fl_want[[0, 5, 129]].any()
    sc.set_identities(cache)
    sc.set_repository(repo)
    dev = torch.device("cuda:0")
    W, E, spare = sc.words, len(eps), 2
    d_ep = torch.from_numpy(np.asarray(eps, np.uint32).view(np.int32).copy()).to(dev)
    d_ing, d_eg, d_fl = _sentinels(dev, E + spare, W)
    torch.cuda.synchronize(dev)
    sc.reach_dev(d_ep, E, d_ing, d_eg, d_fl)
    torch.cuda.synchronize(dev)
    ing = d_ing.cpu().numpy().view(np.uint64).reshape(E + spare, W)
    eg = d_eg.cpu().numpy().view(np.uint64).reshape(E + spare, W)
    fl = d_fl.cpu().numpy()
    assert not ing[outside].any() and not eg[outside].any() and not fl[outside].any()
    in_eps = [eps[a] for a in inside]
    assert np.array_equal(unpack_rows(ing[inside], n), ing_want[in_eps, :n])
    assert np.array_equal(unpack_rows(eg[inside], n), eg_want[in_eps, :n])
    assert np.array_equal(fl[inside], fl_want[in_eps])
    assert not np.any(ing[:E, -1] >> np.uint64(n % 64)) and not np.any(eg[:E, -1] >> np.uint64(n % 64))
    assert np.all(ing[E:] == X.SENTINEL) and np.all(eg[E:] == X.SENTINEL) and np.all(fl[E:] == X.SENTINEL), \
        "written past the last endpoint's row"


def test_gpu_empty_identity_table(sc):
    import torch
    T.check_empty_table(sc, diag_cpu=False)
    # reach on the device with W = 0: flags only.  One-element row tensors,
    # as a tensor without elements has no address to hand over.
    dev = torch.device("cuda:0")
    d_ep = torch.tensor([0, 7], dtype=torch.int32, device=dev)
    d_ing, d_eg, _ = _sentinels(dev, 1, 1)
    d_fl = torch.full((3,), X.SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    sc.reach_dev(d_ep, 2, d_ing, d_eg, d_fl)
    torch.cuda.synchronize(dev)
    assert d_fl.cpu().tolist() == [0, 0, X.SENTINEL]
    assert d_ing.cpu().tolist() == [X.SENTINEL] and d_eg.cpu().tolist() == [X.SENTINEL]
    U.check_match(sc, 65, diag_cpu=False)


def test_gpu_match_long_identities_values_requirements(sc):
    T.check_match_long(sc, diag_cpu=False)


def test_gpu_expand_more_rows_than_chunk_and_grids(sc, cus):
    T.check_expand_many_rows(sc, cus, diag_cpu=False)


def test_gpu_expand_wide_rows_grid_stride(sc, cus):
    T.check_expand_wide_rows(sc, cus, diag_cpu=False)


def test_gpu_fused_entries_more_rows_than_count_grid(sc, cus):
    T.check_fused_many_rows(sc, cus, diag_cpu=False)
