"""KSCHED_COMBINE_SOFT at the C boundary, without a GPU: the constant in the header, the Python binding, the package and the Rust binding with
one value, 0x2000; a single bit outside the predicate, pick and output flags (0x1FF), outside the combine ops (0xE00, which stay spelled from
exactly the three ops) and not 0x1000 (the value callers probe with as unknown); the ABI version and the set of declared functions unchanged
(the flag is detected by its constant and by KSCHED_E_INVAL from an older library); a NULL ctx refused with KSCHED_E_INVAL before anything
touches a device, outputs untouched."""
import ctypes as C
import re

import pytest

from tests.test_uniform_abi import FUNCTIONS, HEADER, SYS_RS, header_functions

SOFT = 0x2000


def test_the_constant_is_0x2000_in_the_header_the_python_binding_and_the_rust_binding(built):
    text = open(HEADER).read()
    sys_rs = open(SYS_RS).read()
    import kube_scheduler_rs_reference_amd as pkg
    from kube_scheduler_rs_reference_amd import _lib
    assert re.search(r"#define\s+KSCHED_COMBINE_SOFT\s+0x2000u\b", text)
    assert _lib.COMBINE_SOFT == SOFT and pkg.COMBINE_SOFT == SOFT
    assert "pub const KSCHED_COMBINE_SOFT: u32 = 0x2000;" in sys_rs
    assert '("KSCHED_COMBINE_SOFT", KSCHED_COMBINE_SOFT as i64)' in sys_rs


def test_it_is_a_single_bit_disjoint_from_every_other_flag_set_and_from_0x1000(built):
    text = open(HEADER).read()
    from kube_scheduler_rs_reference_amd import _lib
    assert bin(SOFT).count("1") == 1
    others = _lib.FIT | _lib.SEL | _lib.TAINT | _lib.PICK_ANY | _lib.WANT_FIT_MASK
    assert others == 0x1FF and not (SOFT & 0x1FF)
    assert _lib.COMBINE_ANY == 0xE00 and not (SOFT & 0xE00), "the modifier is not one of the ops"
    assert re.search(r"#define\s+KSCHED_COMBINE_ANY\s+\(KSCHED_COMBINE_AND \| KSCHED_COMBINE_OR \| KSCHED_COMBINE_ANDNOT\)", text)
    assert SOFT != 0x1000 and not (SOFT & 0x1000)
    assert not re.search(r"#define\s+KSCHED_\w+\s+0x1000u\b", text), "0x1000 stays the value callers probe with as unknown"
    values = [int(v, 16) for v in re.findall(r"#define\s+KSCHED_(?:FIT|SEL|TAINT|PICK_\w+|WANT_FIT_MASK|COMBINE_AND|COMBINE_OR|COMBINE_ANDNOT)\s+(0x[0-9a-fA-F]+)u", text)]
    assert len(values) == 12 and all(not (v & SOFT) for v in values)


def test_the_abi_is_still_7_and_no_function_was_added(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_COMBINE_SOFT\b", text)
    assert re.search(r"#define\s+KSCHED_ABI_VERSION\s+7u", text)
    assert len(FUNCTIONS) == 57 and header_functions() == set(FUNCTIONS)
    from kube_scheduler_rs_reference_amd import _lib
    assert _lib.ABI_VERSION == 7 and set(_lib.SYMBOLS) == set(FUNCTIONS)
    assert _lib.load().ksched_abi_version() == 7
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in open(SYS_RS).read()


@pytest.mark.parametrize("op", [0x200, 0x800], ids=["and", "andnot"])
def test_null_ctx_is_an_error_not_a_crash(built, op):
    import numpy as np
    from kube_scheduler_rs_reference_amd import COMBINE_SOFT, FIT, PICK_UNIFORM, _lib
    flag = op | COMBINE_SOFT
    lib = _lib.load()
    cpu = np.zeros(4, np.int64)
    smp = np.zeros((4, 3), np.uint32)
    mask = np.full((4, 2), 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = np.full(4, 7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.ksched_eval_device(None, 4, p(cpu), p(cpu), None, None, None, 0, FIT | flag, p(mask), None, None, None) == _lib.E_INVAL
    assert lib.ksched_eval_device_pitched(None, 4, p(cpu), p(cpu), None, None, p(smp), 3, FIT | flag | PICK_UNIFORM, p(mask), None, p(out), 2, None) == _lib.E_INVAL
    assert lib.ksched_eval(None, 4, p(cpu), p(cpu), None, None, None, 0, FIT | flag, p(mask), None, None) == _lib.E_INVAL
    assert lib.ksched_pick(None, 4, p(mask), None, p(smp), 3, PICK_UNIFORM | flag, p(out)) == _lib.E_INVAL
    assert lib.ksched_pick_device(None, 4, None, 2, None, None, 3, PICK_UNIFORM | flag, None, None) == _lib.E_INVAL
    assert (out == 7).all() and (mask == 0x5A5A5A5A5A5A5A5A).all()
