"""CPU test of catalog.auto_table_cus for the queued 3-product bound table (`table_queue=True`,
ABI 16): 2-CU steps off the shader-engine grid and the split the config-4 sweep recorded
(profiles/x3b_queue: 162 and 164 table CUs level, 166 and up slower); every call without the
argument returns what it returned before the queue existed."""
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
            gather_bytes=4, k=50, users=50_000, products=3)


def test_queued_bound_table_steps_in_two_cus_and_picks_the_measured_split():
    n = auto_table_cus(_model(64, 64, "fp16x6"), **CFG4, table_queue=True)
    assert n % 2 == 0 and n % 32 != 0
    assert n == 162   # the sweep: 162 / 164 level at 376.9 / 377.3 ms, 160 fixed-grid 393.3, 166 379.4


def test_without_the_argument_the_split_is_the_fixed_grids():
    m = _model(64, 64, "fp16x6")
    assert auto_table_cus(m, **CFG4) == 160                       # the parent's pick: 32-CU steps
    assert auto_table_cus(m, **CFG4, table_queue=False) == 160
    # the argument alone does not make a queue: the job's launches must take the counter
    assert auto_table_cus(m, **CFG4, work_queues=False, table_queue=True) == 160


def test_table_queue_leaves_the_other_table_kernels_alone(monkeypatch):
    m = _model(64, 64, "fp16x6")
    kw = dict(CFG4, products=None)   # the model's own 6-product table (x6n): its own 2-CU steps
    assert auto_table_cus(m, **kw, table_queue=True) == auto_table_cus(m, **kw)
    kw8 = dict(CFG4, gather_bytes=8)   # the exact gather under a 3-product table: engine steps
    assert auto_table_cus(m, **kw8, table_queue=True) == auto_table_cus(m, **kw8)
    monkeypatch.setattr(catalog, "PAIR_WORK_QUEUE", False)
    assert auto_table_cus(m, **CFG4, table_queue=True) == 160


@pytest.mark.parametrize("ncu", [64, 128, 256, 304])
def test_queued_split_stays_inside_the_device(ncu):
    n = auto_table_cus(_model(64, 64, "fp16x6"), **dict(CFG4, ncu=ncu), table_queue=True)
    assert n % 2 == 0 and ncu // 4 <= n <= ncu - 2
