"""GPU: the one-product bound table whose MFMA chains start from S*b1 as srcC (Epi16V in
nais_kernels.hip), through nais_pair_table_bound1_queued and nais_pair_table_bound1_q16_queued.

D = H = 32 and 64, J of 1, 33 and 130 items (a lone item, a chunk's edge, a group's edge), column
blocks of 16, 37 and 512 columns. For every block: each hi word bounds nais_pair_recompute's
(e, e*s) under the widening in force; the fixed-grid and the queued launch write the same bytes;
the q16 words meet the same kernel's hi words. Then a model with b1 = 0 (the srcC tuple is all
zero) and one whose first history row holds a NaN (its table row is NaN in every word, no other
row is touched)."""
import numpy as np
import pytest
import torch

import _q16_format as qf
from test_gpu_ondemand_refine import _model, _recompute, _scales
from test_gpu_one_product_table import _bound1
from test_gpu_q16_table import _q16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_T, W_T = 1061, 512
JS, COLS = (1, 33, 130), (16, 37, 512)


def _check_block(m, items, c0, w, eta, ds):
    J = len(items)
    work = torch.full((1,), 777, dtype=torch.int32, device=DEV)   # the launch zeroes it
    hw = _bound1(m, items, c0, w, None)
    np.testing.assert_array_equal(_bound1(m, items, c0, w, work), hw, err_msg=f"hi J={J} c0={c0} w={w}")
    assert np.all(hw[:, w:] == 0x5A5A5A5A)
    blk = _q16(m, items, c0, w, None)
    work.fill_(777)
    np.testing.assert_array_equal(_q16(m, items, c0, w, work), blk, err_msg=f"q16 J={J} c0={c0} w={w}")
    hw = hw[:, :w]
    eh = (hw << 16).view(np.float32).astype(np.float64)
    esw = hw.view(np.float32).astype(np.float64)
    ph = (hw & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    tiny, up = 2.0 ** -126, 1 + 2.0 ** -7
    if eta is not None:
        eta2 = 1.02 * eta + 2.0 ** -21
        rowsc, colsc = _scales(m, items, c0, w, W_T)
        e6, es6 = (t.astype(np.float64) for t in
                   _recompute(m, items, rowsc, colsc, c0, w, np.arange(J), c0 + np.arange(w)))
        assert np.all(e6 >= eh * (1 - eta) - tiny), (J, c0, w)
        assert np.all(e6 <= eh * up * (1 + eta) + tiny), (J, c0, w)
        radius = (2.0 ** -7 + eta2) * np.abs(esw) + eh * up * (1 + eta) * ds + tiny
        assert np.all(np.abs(es6 - esw) <= radius), (J, c0, w)
    me, ms, qe, qs = qf.dequantise(blk, W_T, w)
    ok = np.isfinite(qe) & np.isfinite(qs)
    elo, ehi = (me - qf.SLACK) * qe.astype(np.float64), (me + 1 + qf.SLACK) * qe.astype(np.float64)
    plo, phi = (ms - qf.SLACK) * qs.astype(np.float64), (ms + 1 + qf.SLACK) * qs.astype(np.float64)
    with np.errstate(all="ignore"):
        assert np.all((elo <= eh * up + tiny)[ok]) and np.all((ehi >= eh)[ok]), (J, c0, w)
        assert np.all((plo <= np.maximum(ph, ph * up) + tiny)[ok]), (J, c0, w)
        assert np.all((phi >= np.minimum(ph, ph * up) - tiny)[ok]), (J, c0, w)
    return hw, blk, ok


@pytest.mark.parametrize("D,H", [(32, 32), (64, 64)])
def test_words_bound_recompute_and_launch_forms_agree(D, H):
    from poi_recommendation_models_amd import catalog
    m = _model(P_T, D, H, emb_std=0.3)
    _, eta, ds = catalog.ondemand_widening(m, products=1)
    assert np.isfinite(eta) and eta <= catalog.PAIR_ONDEMAND_ETA1_MAX, eta
    for J in JS:
        items = torch.arange(5, 5 + J, dtype=torch.int64, device=DEV)
        for c0, w in ((0, 512), (512, 16), (528, 37), (1024, 37)):   # the last: the catalog's ragged end
            assert w in COLS
            _, _, ok = _check_block(m, items, c0, w, eta, ds)
            assert ok.all(), (J, c0, w)


@pytest.mark.parametrize("D,H", [(32, 32), (64, 64)])
def test_zero_bias_and_a_nan_row(D, H):
    from poi_recommendation_models_amd import catalog
    m = _model(P_T, D, H, emb_std=0.3)
    with torch.no_grad():
        m.attn_layer1.bias.zero_()
    _, eta, ds = catalog.ondemand_widening(m, products=1)
    items = torch.arange(5, 5 + 33, dtype=torch.int64, device=DEV)
    clean, cblk, ok = _check_block(m, items, 512, 37, eta, ds)
    assert ok.all()
    m = _model(P_T, D, H, emb_std=0.3)   # a fresh model: nothing cached from the clean one
    with torch.no_grad():
        m.attn_layer1.bias.zero_()
        m.embed_history.weight[int(items[2]), 1] = float("nan")
    hw, blk, ok = _check_block(m, items, 512, 37, None, None)
    e = (hw << 16).view(np.float32)
    assert np.isnan(e[2]).all(), "the NaN row's e"
    assert not ok[2].any(), "the NaN row's q16 scales are not finite"
    # the chunk's scale takes its maximum over the chunk's rows, NaN ignored (fmaxf): the other
    # rows keep their words when the NaN row's own largest entry was not the chunk's
    rest = np.arange(33) != 2
    assert np.isfinite(e[rest]).all() and ok[rest].all()
