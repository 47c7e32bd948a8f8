"""iso_binfit_moments (k_binfit_partial, k_binfit_total) on the device against iso_binfit_moments_host on the same tables:
N and C within 1e-11 relative to max(1, n_live), n_live exact; S = 1, 255, 256, 257 (tiles of 64 stars and a ragged one),
4096 and 4097 (a chunk and a second one), 2 * 4096 + 1 and 3 * 4096 (a third, one of them without a live star); B = 1, 2, 63, 64, 3 x 5 and 8 x 8 cells; H = 1, 8, 9 rows; masked and dead stars,
cells of height 0, no C; a row alone and in a batch, and a repeated call, bit for bit.  No table is larger than 12288 x 64
doubles."""
import numpy as np
import pytest

from isochrones_amd import _binfit_cabi as fc
from tests import _binfit_twin as ft

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    return fc.lib()


def _case(S, B, H):
    dead = sorted({0, S // 3, S - 1}) if S > 3 else ()
    A = ft.random_table(S, B, seed=S + 3 * B, dead=dead)
    lnh = ft.random_lnh(H, B, seed=H + B) if B > 1 else np.random.default_rng(H).normal(size=(H, 1))
    mask = None
    if S > 3:
        mask = np.ones(S, np.int32)
        mask[[1, S // 2, S - 2]] = 0
    return A, lnh, mask


def _against_host(lib, device, A, lnh, mask, pairs=True, guard=False):
    rc, got = ft.call(lib, A, lnh, mask, device=device, pairs=pairs, guard=guard)
    assert rc == 0, lib.iso_binfit_last_error()
    rc, ref = ft.call(lib, A, lnh, mask, pairs=pairs)
    assert rc == 0
    assert np.array_equal(got["n_live"], ref["n_live"])
    scale = np.maximum(1.0, ref["n_live"].astype(np.float64))
    eN = float(np.max(np.abs(got["N"] - ref["N"]) / scale[:, None]))
    eC = float(np.max(np.abs(got["C"] - ref["C"]) / scale[:, None, None])) if pairs else 0.0
    print("S = %d, B = %d, H = %d: device against host, N %.2e, C %.2e (limit 1e-11), n_live %s"
          % (A.shape[1], A.shape[0], lnh.shape[0], eN, eC, ref["n_live"][:3]))
    assert eN <= 1e-11 and eC <= 1e-11
    if pairs:
        assert np.array_equal(got["C"], got["C"].transpose(0, 2, 1))
    else:
        assert (got["C"] == -7.0).all()
    return got, ref


# every S with the largest grid, every B and H at a chunk and a half; 3 x 5 and 8 x 8 are B = 15 and B = 64 to the library
@pytest.mark.parametrize("S, B, H", [(1, 64, 1), (255, 64, 8), (256, 64, 1), (257, 64, 9), (4096, 64, 1), (4097, 64, 9),
                                     (4097, 1, 8), (257, 2, 9), (4097, 63, 1), (300, 15, 8), (1, 1, 1), (4096, 15, 9),
                                     (4097, 2, 1)])
def test_device_matches_the_host_entry(lib, device, S, B, H):
    A, lnh, mask = _case(S, B, H)
    got, ref = _against_host(lib, device, A, lnh, mask)
    # against the long-double twin as well, with both identities
    ft.assert_matches(got, A, lnh, mask)
    if S > 3:
        assert ref["n_live"].max() <= S - 6                             # three dead and three masked stars


@pytest.mark.parametrize("S", [2 * fc.CHUNK + 1, 3 * fc.CHUNK])
@pytest.mark.parametrize("B, H", [(64, 2), (15, 9)])
def test_three_chunks_and_one_without_a_live_star(lib, device, S, B, H):
    """nc = 3: the workspace index (h * nc + chunk) with a third chunk, ragged (one star) and full, and the totals over three
    chunks.  The whole of chunk 1 is masked, so its partial sums are zeros and its live count is 0, between two chunks
    that have dead and masked stars of their own."""
    assert fc.CHUNK == 4096
    A, lnh, mask = _case(S, B, H)
    mask[fc.CHUNK:2 * fc.CHUNK] = 0
    got, ref = _against_host(lib, device, A, lnh, mask, guard=True)
    for k in ("N", "C", "n_live"):
        assert not (got[k] == -7).any(), k
    ft.assert_matches(got, A, lnh, mask)
    assert 0 < ref["n_live"].min() and ref["n_live"].max() <= S - fc.CHUNK - 4
    rc, one = ft.call(lib, A, lnh, mask, device=device, rows=(1, 1), guard=True)
    assert rc == 0
    for k in ("N", "C", "n_live"):
        assert one[k].tobytes() == got[k][1:2].tobytes(), k


@pytest.mark.parametrize("S, B, H", [(4097, 64, 9), (257, 15, 8), (1, 2, 1)])
def test_without_pairs_the_same_counts(lib, device, S, B, H):
    A, lnh, mask = _case(S, B, H)
    got, _ = _against_host(lib, device, A, lnh, mask, pairs=False)
    rc, full = ft.call(lib, A, lnh, mask, device=device)
    assert rc == 0 and full["N"].tobytes() == got["N"].tobytes() and np.array_equal(full["n_live"], got["n_live"])


def test_zero_heights_and_a_row_without_any(lib, device):
    S, B = 700, 8
    A = ft.random_table(S, B, seed=4, sparse=0.0)
    A[1:, 5] = 0.0                                                     # star 5 has weight in cell 0 only
    lnh = np.zeros((5, B))
    lnh[1, 0] = -np.inf
    lnh[2, 0] = np.nan
    lnh[3, 1:] = -np.inf
    lnh[4, :] = -np.inf
    got, _ = _against_host(lib, device, A, lnh, None)
    assert list(got["n_live"]) == [S, S - 1, S - 1, S, 0]
    assert got["N"][1].tobytes() == got["N"][2].tobytes() and got["N"][1, 0] == 0.0
    assert got["N"][3, 0] == S and (got["N"][3, 1:] == 0.0).all() and got["C"][3, 0, 0] == S
    assert (got["N"][4] == 0.0).all() and (got["C"][4] == 0.0).all()
    rc, none = ft.call(lib, A, lnh, np.zeros(S, np.int32), device=device)
    assert rc == 0 and (none["n_live"] == 0).all() and (none["N"] == 0.0).all() and (none["C"] == 0.0).all()


def test_a_row_alone_in_a_batch_and_again(lib, device):
    A, lnh, mask = _case(4097, 64, 9)
    rc, full = ft.call(lib, A, lnh, mask, device=device)
    assert rc == 0
    for first, count in ((4, 1), (0, 1), (8, 1), (2, 5)):
        rc, part = ft.call(lib, A, lnh, mask, device=device, rows=(first, count))
        assert rc == 0
        for key in ("N", "C", "n_live"):
            assert part[key].tobytes() == full[key][first:first + count].tobytes(), (key, first, count)
    rc, again = ft.call(lib, A, lnh, mask, device=device)
    assert rc == 0 and all(again[k].tobytes() == full[k].tobytes() for k in ("N", "C", "n_live"))


def test_the_device_entry_refuses_what_the_host_entry_refuses(lib, device):
    A, lnh, _ = _case(5, 3, 2)
    import torch
    dA = torch.from_numpy(A).to(device)
    p = dA.data_ptr()
    assert lib.iso_binfit_moments(p, 0, 5, p, 2, None, p, None, p, p, None) == fc.ERR_INVALID
    assert "B must be" in lib.iso_binfit_last_error().decode()
    assert lib.iso_binfit_moments(p, 3, 5, p, 2, None, p, None, p, None, None) == fc.ERR_INVALID
    assert "null" in lib.iso_binfit_last_error().decode()
