"""Host code of the Wilson / Granger stage (syncopy_amd/csrc/granger.hip) that only the device ran before, on the CPU
emulator (tests/granger_drive.py): spyhip_zinv with its in-place copy, retry and refusal, the stepped entry points
against spyhip_granger, and the refusals of spyhip_granger.  Small shapes: the emulator runs one OS thread per GPU thread.
The kernels themselves are checked in tests/test_emu_kernels.py."""
import ctypes as C

import numpy as np

import build_emu
import granger_drive as GD


def _inv_launch(n, blocked):
    """(threads, LDS bytes) of the inverse launch the route gives (n, blocked) out of place on the default chip"""
    o, _ = GD._ask(GD.route().wr_inv, 4, n, int(blocked), 1, C.c_ulonglong(GD.chip()[1]))
    return o[1], o[2]


def test_zinv_in_place_equals_out_of_place():
    """n = 32, two matrices: the block kernel alone; dst == src inverts from the copy kept in the arena, same bits."""
    rng = np.random.default_rng(32)
    B, n = 2, 32
    A = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n)) + 3 * np.sqrt(n) * np.eye(n)
    out = np.zeros_like(A)
    GD.lib().emu_launch_log_reset()
    assert GD.zinv(A, out) == 0
    log = build_emu.launches(GD.lib())
    assert [tuple(r) for r in log] == [(B, 1, 1, _inv_launch(n, True)[0], 1, 1, _inv_launch(n, True)[1])]
    np.testing.assert_allclose(out @ A, np.tile(np.eye(n), (B, 1, 1)), atol=1e-10)
    same = A.copy()
    assert GD.zinv(same) == 0
    assert np.array_equal(same.view(np.uint64), out.view(np.uint64))


def test_zinv_retries_with_the_pivoted_kernel_and_refuses_a_singular_matrix():
    """An anti-diagonal permutation matrix: every leading block is singular, so the block kernel flags a tiny pivot and the
    whole batch is repeated with the partially pivoted kernel, which returns the transpose; a zero matrix is refused (-7)."""
    B, n = 2, 32
    P = np.zeros((B, n, n), complex)
    P[:] = np.eye(n)[::-1]
    for dst in (np.zeros_like(P), None):              # out of place, in place
        src = P.copy()
        GD.lib().emu_launch_log_reset()
        assert GD.zinv(src, dst) == 0
        log = build_emu.launches(GD.lib())
        assert [tuple(r[[0, 3, 6]]) for r in log] == [(B, *_inv_launch(n, True)), (B, *_inv_launch(n, False))]
        assert _inv_launch(n, True) != _inv_launch(n, False)
        assert np.array_equal(src if dst is None else dst, P.transpose(0, 2, 1))
    Z = np.zeros((B, n, n), complex)
    assert GD.zinv(Z, np.zeros_like(Z)) == -7


def _csd(F, n, seed):
    """a well-conditioned Hermitian positive definite spectrum, complex64 (no regularisation step is taken)"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(F, n, n)) + 1j * rng.normal(size=(F, n, n))
    return (X @ X.conj().transpose(0, 2, 1) / n + 2 * np.eye(n)).astype(np.complex64)


def test_stepped_entry_points_equal_spyhip_granger_bit_for_bit():
    """One shard: spyhip_wilson_cond, _init, _psi0, then _g, _plus, _update per iteration, then _finish, driven by
    granger_sharded of syncopy_amd/connectivity/wilson_sharded.py, against spyhip_granger: n = 3, F = 9 (L = 16), two
    iterations (unconverged).  Both run the same step functions of granger.hip; spyhip_granger carves its arrays out of the
    context's arena and swaps psi, the stepped entry points take the caller's arrays and copy."""
    import torch
    from syncopy_amd.connectivity.wilson_sharded import granger_sharded
    F, n = 9, 3
    csd = _csd(F, n, 9)
    G, H, Sigma, info = GD.granger(csd, niter=2)
    assert info[0] == 0 and GD.last_iterations() == 2 and info[2] == 0
    Gs, meta, Hs, Ss = granger_sharded(torch.from_numpy(csd), 0, F, GD.sharded_prims(), niter=2)
    assert not meta["converged"] and meta["iterations"] == 2 and meta["reg. factor"] == 0
    assert (meta["max rel. err"], meta["initial cond. num"]) == (info[1], info[3])
    assert np.array_equal(Gs.numpy().view(np.uint32), G.view(np.uint32))
    assert np.array_equal(Hs.numpy().view(np.uint64), H.view(np.uint64))
    assert np.array_equal(Ss.numpy().view(np.uint64), Sigma.view(np.uint64))
    assert np.isfinite(G).all() and np.abs(H).max() > 0


def test_spyhip_granger_refusals():
    """Null arguments and fewer than three frequencies: -1, before anything is allocated.  (The third refusal, -3 for a
    lag-domain length without a radix schedule, cannot be reached with a 32-bit length: plus_plan takes any prime factor
    and gives up only beyond 24 factors, and with 4 taken first the shortest such length is 3^25.)"""
    L, c = GD.lib(), GD.ctx()
    csd = _csd(9, 3, 1)
    G, H, S, info = np.zeros((9, 3, 3), np.float32), np.zeros((9, 3, 3), complex), np.zeros((3, 3), complex), np.zeros(4)
    ip = info.ctypes.data_as(C.POINTER(C.c_double))
    args = [c, GD.ptr(csd), 9, 3, 5e-6, 2, 1e4, 1e-1, GD.ptr(G), GD.ptr(H), GD.ptr(S), ip]
    for k in (0, 1, 8, 11):
        bad = list(args)
        bad[k] = None
        assert L.spyhip_granger(*bad) == -1, k
    assert L.spyhip_granger(*args[:2], 2, 3, *args[4:]) == -1
    assert L.spyhip_granger(*args[:3], 0, *args[4:]) == -1
    assert not G.any() and not info.any()
