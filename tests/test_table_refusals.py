"""The packer's refusals, without a GPU: pvt_scene_lean_check runs pack_scene on the host, so every malformed table the
GPU tests hand to a pvt_scene_create* entry (tests/broken_tables.py) must meet the same code and message here -- but for
the cases broken_tables.LEAN_CHECK_CANNOT names, whose refusal is create_scene's own or depends on the entry's level."""
import ctypes as C

import pytest

from pvtrace_amd.engine import compile_scene, native
from tests import broken_tables as BT


def lean_check(st, x=None, ph=None, rs=None, fr=None, mp=None):
    """pvt_scene_lean_check on the structs -> (return code, pvt_last_error when refused)."""
    lib = native.load_library()
    lean = C.c_int32(0)
    rc = lib.pvt_scene_lean_check(C.byref(st), *(None if s is None else C.byref(s) for s in (x, ph, rs, fr, mp)),
                                  C.byref(lean))
    return rc, (lib.pvt_last_error().decode() if rc != 0 else "")


RAN = set()   # the messages of the BROKEN_TABLES cases that went through pvt_scene_lean_check


@pytest.mark.parametrize("case", range(len(BT.BROKEN_TABLES)), ids=[m for _, _, _, m in BT.BROKEN_TABLES])
def test_lean_check_refuses_broken_tables_like_scene_create(case, built):
    scene, breaks, code, message = BT.BROKEN_TABLES[case]
    if message in BT.LEAN_CHECK_CANNOT:
        return   # (named there with its reason; tests/test_gpu_parity.py holds it)
    compiled = compile_scene(BT.SCENES[scene]())
    st, keep = native.scene_tables_struct(compiled)
    assert lean_check(st)[0] == 0   # the scene as compiled is accepted
    breaks(st, keep, compiled)
    assert lean_check(st) == (code, message)
    RAN.add(message)


def test_every_case_ran_but_the_ones_named_with_a_reason():
    """(after the cases above) the exclusion list holds cases of the list only, each with a reason, and nothing else was
    left out."""
    messages = [m for _, _, _, m in BT.BROKEN_TABLES]
    assert set(BT.LEAN_CHECK_CANNOT) <= set(messages)
    assert all(reason.strip() for reason in BT.LEAN_CHECK_CANNOT.values())
    assert RAN == set(messages) - set(BT.LEAN_CHECK_CANNOT)
    assert len(RAN) == len(messages) - len(BT.LEAN_CHECK_CANNOT) == 20


@pytest.mark.parametrize("case", sorted(BT.INDEX_BREAKS))
def test_lean_check_refuses_each_broken_index_table(case, built):
    compiled = compile_scene(BT.index_scene())
    st, keep = native.scene_tables_struct(compiled)
    xt, arrays = BT.index_tables(compiled, BT.index_edit())
    assert lean_check(st, x=xt)[0] == 0
    edit, message = BT.INDEX_BREAKS[case]
    xt, arrays = BT.index_tables(compiled, edit)
    rc, err = lean_check(st, x=xt)
    assert rc == BT.INVALID and message in err, (case, rc, err)


def test_lean_check_refuses_bad_roughness(built):
    compiled = compile_scene(BT.rough_scene())
    st, keep = native.scene_tables_struct(compiled)
    rt, alpha = BT.surface_tables(0.0)
    assert lean_check(st, rs=rt)[0] == 0
    for bad in BT.BAD_ROUGHNESS:
        rt, alpha = BT.surface_tables(bad)
        assert lean_check(st, rs=rt) == (BT.INVALID, "surface tables: roughness must be finite and within [0, 1]"), bad


def test_lean_check_refuses_each_malformed_field_table_with_its_own_message(built):
    compiled = compile_scene(BT.field_scene())
    st, keep = native.scene_tables_struct(compiled)
    ft, held = BT.field_tables()
    assert lean_check(st, fr=ft)[0] == 0
    messages = {}
    for what, change in BT.FIELD_BREAKS.items():
        ft, held = BT.field_tables(**change)
        rc, msg = lean_check(st, fr=ft)
        assert rc == BT.INVALID and "field tables" in msg, (what, rc, msg)
        messages[what] = msg
    assert len(set(messages.values())) == len(messages), messages


def test_lean_check_refuses_each_malformed_map_table_with_its_own_message(built):
    compiled = compile_scene(BT.map_scene())
    st, keep = native.scene_tables_struct(compiled)
    mt, held = BT.map_tables()
    assert lean_check(st, mp=mt)[0] == 0
    messages = {}
    for what, change in BT.MAP_BREAKS.items():
        mt, held = BT.map_tables(**change)
        rc, msg = lean_check(st, mp=mt)
        assert rc == BT.INVALID and "map tables" in msg, (what, rc, msg)
        messages[what] = msg
    assert len(set(messages.values())) == len(messages), messages
