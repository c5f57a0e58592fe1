"""CPU test of catalog.auto_table_cus's `absepi` keyword (the q16 route with the |z| epilogue in
the table kernel, profiles/absepi): without it, and with absepi=False, every signature of
test_cost_model_lean's grid returns the value recorded before the `lean` keyword existed, and the
grid under lean=True returns what lean=True alone returns; with it only the q16 route at the shape
that takes the new epilogue (padded D = 64, 32 < H <= 64) may answer differently, and there the
gather keeps at least three whole XCDs."""
import pytest

from poi_recommendation_models_amd.catalog import auto_table_cus
from test_cost_model_lean import BEFORE, _grid
from test_cost_model_q16 import CFG4, _model


def test_the_default_reproduces_every_value():
    assert [auto_table_cus(m, **c) for m, c in _grid()] == BEFORE
    assert [auto_table_cus(m, **c, absepi=False) for m, c in _grid()] == BEFORE
    lean = [auto_table_cus(m, **c, lean=True) for m, c in _grid()]
    assert [auto_table_cus(m, **c, lean=True, absepi=False) for m, c in _grid()] == lean
    # the keyword rides on `lean`: alone it changes nothing
    assert [auto_table_cus(m, **c, absepi=True) for m, c in _grid()] == BEFORE


def test_absepi_applies_to_the_q16_route_and_its_shape_alone():
    moved = 0
    for m, c in _grid():
        lean = auto_table_cus(m, **c, lean=True)
        n = auto_table_cus(m, **c, lean=True, absepi=True)
        H, din = m.attn_layer1.weight.shape
        if n != lean:
            moved += 1
            assert c.get("q16") and c.get("table_queue") and c.get("products") == 1 and c["gather_bytes"] == 4
            assert din == 64 and 32 < H <= 64 and c.get("work_queues", True) and not c.get("prior")
            assert c["ncu"] - n >= 3 * (c["ncu"] // 8), (c, n)
    assert moved   # the grid does reach the route (128 CUs: 58 against 60)


@pytest.mark.parametrize("ncu", [256, 304])
def test_config4_split(ncu):
    """config 4: 160 of 256 CUs still -- the streams are level there and the gather does not run
    on fewer than three whole XCDs (profiles/absepi)."""
    m = _model(64, 64, "fp16x6")
    n = auto_table_cus(m, **dict(CFG4, ncu=ncu), products=1, table_queue=True, q16=True, lean=True, absepi=True)
    assert ncu - n >= 3 * (ncu // 8) and n % 2 == 0
    if ncu == 256:
        assert n == 160
