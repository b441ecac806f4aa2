"""Index arithmetic of the folded cross-attention (no GPU): kh, k_fold and the column of (head, key) as rtv_cross_fold_dims and
tests/cross_fold_cases.fold_dims state them, against a NumPy evaluation of the identity the fold rests on,
    ao . Wo^T = sum_h P_h . (V_h . Wo_h^T) = P_all . ca_vo^T,
with P_all [rows, k_fold] and ca_vo [d, k_fold] laid out by exactly those numbers and zeros in every padding column."""
import ctypes

import numpy as np
import pytest

import cross_fold_cases as cf


def _dims(H, text_rows):
    from realtime_video_amd import _lib
    kh, kf = ctypes.c_int(-1), ctypes.c_int(-1)
    ok = _lib.load().rtv_cross_fold_dims(H, text_rows, ctypes.byref(kh), ctypes.byref(kf))
    return bool(ok), kh.value, kf.value


@pytest.mark.parametrize("H,text_rows,kh,k_fold", [(3, 5, 8, 64), (2, 64, 72, 192), (3, 64, 72, 256), (12, 64, 72, 896),
                                                   (40, 64, 72, 2880), (2, 7, 8, 64), (2, 8, 16, 64), (40, 1, 8, 320)])
def test_fold_dims(H, text_rows, kh, k_fold):
    assert _dims(H, text_rows) == (True, kh, k_fold)
    assert cf.fold_dims(H, text_rows) == (kh, k_fold)
    assert kh % 8 == 0 and kh >= text_rows + 1 and k_fold % 64 == 0 and H * kh <= k_fold < H * kh + 64


def test_fold_dims_cut_and_refusals():
    from realtime_video_amd import _lib
    import re
    kh_max = int(re.search(r"^#define\s+RTV_CROSS_FOLD_KH_MAX\s+(\d+)", _lib._read(_lib.CROSS_FOLD_HEADER), flags=re.M).group(1))
    assert kh_max % 8 == 0 and 8 <= kh_max <= 128
    assert _dims(40, kh_max - 1)[:2] == (True, kh_max)                 # the longest prompt the fold takes
    assert _dims(40, kh_max)[:2] == (False, kh_max + 8)                # one more row: another 8 columns per head, beyond the cut
    assert _dims(40, 0)[0] is False and _dims(0, 5)[0] is False
    assert _lib.load().rtv_cross_fold_dims(3, 5, None, None) == 1      # the outputs are optional


def test_identity_in_the_folded_layout():
    """H = 3, text_rows = 5 (6 keys per head in 8 columns, 24 columns padded to 64): random P, V, Wo in float64."""
    H, text_rows, M = 3, 5, 7
    d, keys = 128 * H, text_rows + 1
    kh, kf = cf.fold_dims(H, text_rows)
    rng = np.random.default_rng(0)
    p = rng.random((M, H, keys))
    p /= p.sum(-1, keepdims=True)
    v, wo = rng.standard_normal((keys, H, 128)), rng.standard_normal((d, d))
    ao = np.einsum("mhk,khd->mhd", p, v).reshape(M, d)
    p_all, vo = np.zeros((M, kf)), np.zeros((d, kf))
    for h in range(H):
        for t in range(keys):
            col = h * kh + t                                           # the column of (h, t)
            p_all[:, col] = p[:, h, t]
            vo[:, col] = wo[:, h * 128:(h + 1) * 128] @ v[t, h]
    assert np.count_nonzero(p_all.any(0)) == H * keys == np.count_nonzero(vo.any(0))
    np.testing.assert_allclose(p_all @ vo.T, ao @ wo.T, rtol=1e-12, atol=1e-12)
