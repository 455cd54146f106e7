"""KSCHED_APPLY_WHILE_FIT at the C boundary, without a GPU: the same value in the header, _lib and the Rust raw binding, no symbol added
and the ABI version unchanged (the flag is detected by its constant and by KSCHED_E_INVAL from an older library), NULL handles refused
without a crash."""
import ctypes as C
import os
import re

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ksched.h")
SYS_RS = os.path.join(ROOT, "rust", "src", "ksched_sys.rs")


def test_the_three_faces_carry_the_same_value():
    from kube_scheduler_rs_reference_amd import _lib
    assert re.search(r"^#define KSCHED_APPLY_WHILE_FIT 0x08u\s*$", open(HEADER).read(), flags=re.M)
    assert _lib.APPLY_WHILE_FIT == 0x08
    sys_rs = open(SYS_RS).read()
    assert re.search(r"pub const KSCHED_APPLY_WHILE_FIT: u32 = 0x08;", sys_rs)
    assert '("KSCHED_APPLY_WHILE_FIT", KSCHED_APPLY_WHILE_FIT as i64)' in sys_rs
    # the values the existing tests probe with as unknown flags stay free
    assert _lib.APPLY_WHILE_FIT not in (0x04, 0x80)
    assert _lib.APPLY_WHILE_FIT & (_lib.APPLY_FIRST_PER_NODE | _lib.APPLY_RELEASE) == 0


def test_no_symbol_was_added_and_the_abi_is_7(built):
    from kube_scheduler_rs_reference_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(ksched_[a-z_0-9]+)\s*\(", text))
    assert len(names) == 57
    assert "#define KSCHED_ABI_VERSION 7u" in open(HEADER).read()
    assert _lib.load().ksched_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert len(_lib.SYMBOLS) == 57


def test_null_handles_with_the_flag_are_errors_not_crashes(built):
    from kube_scheduler_rs_reference_amd import _lib
    lib = _lib.load()
    W = _lib.APPLY_WHILE_FIT
    assert lib.ksched_apply_bindings_device(None, 0, None, None, None, None, W, None, None) == _lib.E_INVAL
    assert lib.ksched_apply_bindings_device(None, 4, None, None, None, None, W | _lib.APPLY_RELEASE, None, None) == _lib.E_INVAL
    f, l = lib.ksched_apply_bindings_sharded, lib.ksched_apply_bindings_sharded_local
    assert f(None, None, 0, 0, None, None, None, None, W, None, None) == _lib.E_INVAL
    assert f(None, None, 4, 0, None, None, None, None, W | _lib.APPLY_FIRST_PER_NODE, None, None) == _lib.E_INVAL
    assert l(None, None, 1, None, None, None, None, None, None, W, None, None) == _lib.E_INVAL
    nulls = (C.c_void_p * 2)()
    counts, lows = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(0, 0)
    vp = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    assert l(vp(nulls), vp(nulls), 2, vp(counts), vp(lows), vp(nulls), vp(nulls), vp(nulls), None, W, None, None) == _lib.E_INVAL
