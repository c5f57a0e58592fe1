"""CPU test of catalog.auto_table_cus's q16 branch (`q16=True` with `products=1` and
`table_queue=True`, ABI 20): 2.25 gathered bytes per pair, the q16 table rate and gather margin,
and the split the config-4 sweep recorded (profiles/q16: 160 table CUs lowest in three alternating
rounds, 283.1-283.8 ms; 158 284.2-284.5, 162 286.2-286.7, 156 and 164 further off). Every call
without the argument, and every call where it does not apply, returns what it did."""
import types

import pytest
import torch

from poi_recommendation_models_amd import catalog
from poi_recommendation_models_amd.catalog import auto_table_cus, bounded_gather_cu_seconds


def _model(d, h, precision):
    return types.SimpleNamespace(attn_layer1=types.SimpleNamespace(weight=torch.empty(h, d)),
                                 precision=precision)


# config 4 on the on-demand route, as catalog._score_topk_pairs calls it
CFG4 = dict(J=100_000, NC=100_000, entries=5_030_351, ncu=256, prior=False, block_bytes=100_000 * 512 * 4,
            gather_bytes=4, k=50, users=50_000)


def test_q16_branch_picks_the_measured_split():
    m = _model(64, 64, "fp16x6")
    n = auto_table_cus(m, **CFG4, products=1, table_queue=True, q16=True)
    assert n == 160
    # fewer gathered bytes: the tables get CUs the hi-word gather needed
    assert n > auto_table_cus(m, **CFG4, products=1, table_queue=True)


def test_existing_signatures_return_their_old_values():
    m = _model(64, 64, "fp16x6")
    assert auto_table_cus(m, **CFG4, products=1, table_queue=True) == 122        # tests/test_cost_model_one_product.py
    assert auto_table_cus(m, **CFG4, products=3, table_queue=True) == 162        # tests/test_cost_model_queue.py
    assert auto_table_cus(m, **CFG4, products=1, table_queue=True, q16=False) == 122
    # the three-term fit at its default is the hi-word one
    assert bounded_gather_cu_seconds(5_030_351, 100_000, 50_000, 50) == \
        bounded_gather_cu_seconds(5_030_351, 100_000, 50_000, 50, 4.0)
    assert bounded_gather_cu_seconds(5_030_351, 100_000, 50_000, 50, 2.25) < \
        bounded_gather_cu_seconds(5_030_351, 100_000, 50_000, 50)


def test_q16_is_ignored_where_the_one_product_queue_does_not_run(monkeypatch):
    m = _model(64, 64, "fp16x6")
    for kw in (dict(products=3, table_queue=True), dict(products=1), dict(products=1, table_queue=False), dict(),
               dict(products=1, table_queue=True, work_queues=False)):
        assert auto_table_cus(m, **CFG4, **kw, q16=True) == auto_table_cus(m, **CFG4, **kw), kw
    kw8 = dict(CFG4, gather_bytes=8)   # the exact gather: not the bound route
    assert auto_table_cus(m, **kw8, products=1, table_queue=True, q16=True) == \
        auto_table_cus(m, **kw8, products=1, table_queue=True)
    for mm in (_model(64, 128, "fp16x6"), _model(128, 64, "fp16x6")):   # no one-product instance
        assert auto_table_cus(mm, **CFG4, products=1, table_queue=True, q16=True) == \
            auto_table_cus(mm, **CFG4, products=1, table_queue=True)
    assert auto_table_cus(m, **dict(CFG4, prior=True), products=1, table_queue=True, q16=True) == \
        auto_table_cus(m, **dict(CFG4, prior=True), products=1, table_queue=True)
    monkeypatch.setattr(catalog, "PAIR_WORK_QUEUE", False)
    assert auto_table_cus(m, **CFG4, products=1, table_queue=True, q16=True) == \
        auto_table_cus(m, **CFG4, products=1)


@pytest.mark.parametrize("ncu", [64, 128, 256, 304])
def test_q16_split_stays_inside_the_device(ncu):
    n = auto_table_cus(_model(64, 64, "fp16x6"), **dict(CFG4, ncu=ncu), products=1, table_queue=True, q16=True)
    assert n % 2 == 0 and ncu // 4 <= n <= ncu - 2


@pytest.mark.parametrize("D,H", [(32, 32), (40, 40), (64, 32)])
def test_q16_split_other_shapes(D, H):
    n = auto_table_cus(_model(D, H, "fp16x6"), **CFG4, products=1, table_queue=True, q16=True)
    assert n % 2 == 0 and 64 <= n <= 160      # less matrix work per pair than D = H = 64: no more CUs
