"""CPU test of catalog.auto_table_cus's `lean` keyword (the q16 route after the cut of its VALU
work, profiles/lean): without it, and with lean=False, every signature of the grid below returns
the value recorded from the function before the keyword existed; with it only the q16 route may
answer differently, and there the gather keeps at least three whole XCDs."""
import pytest

from poi_recommendation_models_amd.catalog import auto_table_cus
from test_cost_model_q16 import CFG4, _model

MODELS = ((64, 64, "fp16x6"), (32, 32, "fp16x6"), (64, 128, "fp16x6"), (128, 64, "fp16x6"), (64, 64, "fp32"),
          (64, 64, "fp16x3"))
NCUS = (256, 128, 304)
KWS = ({}, dict(products=1, table_queue=True), dict(products=3, table_queue=True),
       dict(products=1, table_queue=True, q16=True), dict(products=1, table_queue=True, q16=True, work_queues=False),
       dict(products=1, q16=True), dict(prior=True, products=1, table_queue=True, q16=True))
GBS = (4, 8)
# auto_table_cus over MODELS x NCUS x KWS x GBS (in that nesting) at the commit before `lean`
BEFORE = [
    190, 152, 122, 192, 162, 128, 160, 192, 192, 192, 192, 192, 224, 160, 76, 56, 40, 80, 60, 48, 58, 80, 96, 80,
    96, 80, 96, 64, 234, 192, 160, 228, 204, 190, 202, 228, 266, 228, 266, 228, 266, 190, 148, 144, 112, 128, 132,
    128, 108, 128, 160, 128, 160, 128, 160, 128, 36, 32, 32, 32, 32, 32, 32, 32, 48, 32, 48, 32, 64, 32, 196, 192,
    160, 190, 180, 190, 156, 190, 190, 190, 190, 190, 190, 190, 218, 192, 224, 192, 196, 160, 224, 192, 224, 192,
    224, 192, 224, 192, 94, 80, 96, 96, 82, 64, 96, 96, 96, 96, 96, 96, 96, 80, 264, 240, 266, 266, 242, 190, 266,
    266, 266, 266, 266, 266, 266, 228, 218, 192, 224, 192, 196, 160, 224, 192, 224, 192, 224, 192, 224, 192, 94,
    80, 96, 96, 82, 64, 96, 96, 96, 96, 96, 96, 96, 80, 264, 240, 266, 266, 242, 190, 266, 266, 266, 266, 266, 266,
    266, 228, 192, 192, 122, 192, 162, 128, 160, 192, 192, 192, 192, 192, 224, 160, 96, 80, 40, 80, 60, 48, 58, 80,
    96, 80, 96, 80, 96, 64, 266, 228, 160, 228, 204, 190, 202, 228, 266, 228, 266, 228, 266, 190, 160, 128, 122,
    192, 162, 128, 160, 192, 192, 192, 192, 192, 224, 160, 64, 48, 40, 80, 60, 48, 58, 80, 96, 80, 96, 80, 96, 64,
    190, 190, 160, 228, 204, 190, 202, 228, 266, 228, 266, 228, 266, 190]


def _grid():
    for D, H, prec in MODELS:
        m = _model(D, H, prec)
        for ncu in NCUS:
            for kw in KWS:
                for gb in GBS:
                    c = dict(CFG4, ncu=ncu)
                    c.update(kw)
                    c["gather_bytes"] = gb
                    yield m, c


def test_the_default_reproduces_every_value():
    got = [auto_table_cus(m, **c) for m, c in _grid()]
    assert got == BEFORE
    assert [auto_table_cus(m, **c, lean=False) for m, c in _grid()] == BEFORE


def test_lean_applies_to_the_q16_route_alone():
    for (m, c), before in zip(_grid(), BEFORE):
        n = auto_table_cus(m, **c, lean=True)
        q16_route = n != before
        if q16_route:
            assert c.get("q16") and c.get("table_queue") and c.get("products") == 1 and c["gather_bytes"] == 4
        if c.get("q16") and auto_table_cus(m, **dict(c, q16=False)) != before:   # the q16 route took this job
            assert c["ncu"] - n >= 3 * (c["ncu"] // 8), (c, n)


@pytest.mark.parametrize("ncu", [256, 304])
def test_config4_split(ncu):
    """config 4: the table stream stays at 160 of 256 CUs -- the tables still set the step there
    and the gather does not run on fewer than three whole XCDs (profiles/lean)."""
    m = _model(64, 64, "fp16x6")
    n = auto_table_cus(m, **dict(CFG4, ncu=ncu), products=1, table_queue=True, q16=True, lean=True)
    assert ncu - n >= 3 * (ncu // 8) and n % 2 == 0
    if ncu == 256:
        assert n == 160
