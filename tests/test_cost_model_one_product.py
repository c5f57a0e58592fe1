"""CPU test of catalog.auto_table_cus for the queued one-product-logit bound table (`products=1`
with `table_queue=True`, ABI 17): its own table rate in 2-CU steps, and the split the config-4
sweep recorded (profiles/x1b: 120 / 122 / 124 table CUs level at 310-311 ms, 118 and below on the
tables' cliff, 128 and up slower). Calls without the pair of arguments return what they did."""
import types

import pytest
import torch

from poi_recommendation_models_amd import catalog
from poi_recommendation_models_amd.catalog import auto_table_cus


def _model(d, h, precision):
    return types.SimpleNamespace(attn_layer1=types.SimpleNamespace(weight=torch.empty(h, d)),
                                 precision=precision)


# config 4 on the on-demand route, as catalog._score_topk_pairs calls it
CFG4 = dict(J=100_000, NC=100_000, entries=5_030_351, ncu=256, prior=False, block_bytes=100_000 * 512 * 4,
            gather_bytes=4, k=50, users=50_000)


def test_one_product_table_gets_fewer_cus_than_three_products_and_the_measured_split():
    m = _model(64, 64, "fp16x6")
    n1 = auto_table_cus(m, **CFG4, products=1, table_queue=True)
    n3 = auto_table_cus(m, **CFG4, products=3, table_queue=True)
    assert n3 == 162                       # unchanged (tests/test_cost_model_queue.py)
    assert n1 % 2 == 0 and n1 < n3
    assert n1 == 122   # the sweep: 120 / 122 / 124 level (309.9 / 310.2 / 310.7 ms), 118 315.3, 128 311.2


def test_products_one_without_the_queue_is_still_the_fp32_kernels_model():
    """products == 1 has always meant the exact-fp32 table kernel (1.3e14 FLOP/s): only the given
    argument together with `table_queue` (and a job whose launches take the counter) is the
    one-product bound table."""
    m6, m32 = _model(64, 64, "fp16x6"), _model(64, 64, "fp32")
    kw8 = dict(CFG4, gather_bytes=8)
    fp32 = auto_table_cus(m32, **kw8)                                     # derived from the model
    assert auto_table_cus(m32, **kw8, table_queue=True) == fp32
    assert auto_table_cus(m6, **kw8, products=1) == fp32                  # given, no queue
    assert auto_table_cus(m6, **kw8, products=1, table_queue=True) == fp32   # the exact gather: not the bound route
    assert auto_table_cus(m6, **CFG4, products=1) == auto_table_cus(m6, **CFG4, products=1, table_queue=False)
    assert auto_table_cus(m6, **CFG4, products=1, work_queues=False, table_queue=True) == \
        auto_table_cus(m6, **CFG4, products=1)


def test_knob_and_shapes_outside_the_kernel(monkeypatch):
    m = _model(64, 64, "fp16x6")
    plain = auto_table_cus(m, **CFG4, products=1)
    # hidden > 64 and embed_dim 128 have no one-product instance
    assert auto_table_cus(_model(64, 128, "fp16x6"), **CFG4, products=1, table_queue=True) == \
        auto_table_cus(_model(64, 128, "fp16x6"), **CFG4, products=1)
    assert auto_table_cus(_model(128, 64, "fp16x6"), **CFG4, products=1, table_queue=True) == \
        auto_table_cus(_model(128, 64, "fp16x6"), **CFG4, products=1)
    assert auto_table_cus(m, **dict(CFG4, prior=True), products=1, table_queue=True) == \
        auto_table_cus(m, **dict(CFG4, prior=True), products=1)
    monkeypatch.setattr(catalog, "PAIR_WORK_QUEUE", False)
    assert auto_table_cus(m, **CFG4, products=1, table_queue=True) == plain


@pytest.mark.parametrize("ncu", [64, 128, 256, 304])
def test_one_product_split_stays_inside_the_device(ncu):
    n = auto_table_cus(_model(64, 64, "fp16x6"), **dict(CFG4, ncu=ncu), products=1, table_queue=True)
    assert n % 2 == 0 and ncu // 4 <= n <= ncu - 2


@pytest.mark.parametrize("D,H", [(32, 32), (40, 40), (64, 32)])
def test_one_product_split_other_shapes(D, H):
    n = auto_table_cus(_model(D, H, "fp16x6"), **CFG4, products=1, table_queue=True)
    assert n % 2 == 0 and 64 <= n <= 122      # less matrix work per pair than D = H = 64: no more CUs
