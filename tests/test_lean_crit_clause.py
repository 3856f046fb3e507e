"""The last clause of the lean proof (pvt_scene_pack.h: prove_lean): every entry of the packed cosine-threshold table is a
number, because the lean kernels decide total reflection by that threshold alone -- the arm that evaluates acos and asin
is not compiled into them.  PVT_NO_COS_THRESHOLD, read when the tables are packed, writes NaN where a finite threshold
would stand (the generic kernels then evaluate the reference's own expression: same results); a scene that is lean in
every other respect must then be refused, with this clause named, and run the generic family.  Host only."""
import pytest

from pvtrace_amd.engine import compile_scene, native
from tests import scenes

CLAUSE = "an index pair without a proven critical-angle threshold"


@pytest.fixture
def built_library():
    if not native.library_built():
        pytest.skip("library not built")


@pytest.mark.parametrize("build", [scenes.touching_boxes, scenes.lsc_equivalent], ids=["touching_boxes", "lsc_equivalent"])
def test_a_nan_threshold_refuses_the_scene_and_names_the_clause(build, built_library, monkeypatch):
    compiled = compile_scene(build())
    monkeypatch.delenv("PVT_NO_COS_THRESHOLD", raising=False)
    assert native.lean_kind(compiled) == 2 and native.lean_refusal(compiled) is None   # numeric thresholds: lean
    monkeypatch.setenv("PVT_NO_COS_THRESHOLD", "1")
    assert native.lean_kind(compiled) == 0
    assert native.lean_refusal(compiled) == CLAUSE
    monkeypatch.delenv("PVT_NO_COS_THRESHOLD")
    assert native.lean_kind(compiled) == 2                                             # and lean again without the switch


def test_other_refusals_name_their_own_clause(built_library, monkeypatch):
    monkeypatch.delenv("PVT_NO_COS_THRESHOLD", raising=False)
    why = native.lean_refusal(compile_scene(scenes.mesh_lsc()))
    assert why is not None and why != CLAUSE
