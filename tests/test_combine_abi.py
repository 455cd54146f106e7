"""KSCHED_COMBINE_AND / _OR / _ANDNOT at the C boundary, without a GPU: the constants in the header, the Python binding, the package and the
Rust binding with one value each; three single bits that no other flag of ksched_eval* uses, none of them 0x1000 (the value callers probe
with as unknown); the ABI version and the set of declared functions unchanged (the flags are detected by their constants and by
KSCHED_E_INVAL from an older library); a NULL ctx refused with KSCHED_E_INVAL before anything touches a device, outputs untouched."""
import ctypes as C
import re

import pytest

from tests.test_uniform_abi import FUNCTIONS, HEADER, SYS_RS, header_functions

VALUES = {"COMBINE_AND": 0x200, "COMBINE_OR": 0x400, "COMBINE_ANDNOT": 0x800}
OTHER_FLAGS = ("FIT", "SEL", "TAINT", "PICK_SAMPLED", "PICK_BESTFIT", "WANT_FIT_MASK", "PICK_UNIFORM", "PICK_SPREAD", "PICK_PACK")


def test_the_constants_are_0x200_0x400_0x800_in_the_header_the_python_binding_and_the_rust_binding(built):
    text = open(HEADER).read()
    sys_rs = open(SYS_RS).read()
    import kube_scheduler_rs_reference_amd as pkg
    from kube_scheduler_rs_reference_amd import _lib, _marshal
    for name, value in VALUES.items():
        assert re.search(r"#define\s+KSCHED_%s\s+0x%xu\b" % (name, value), text), name
        assert getattr(_lib, name) == value and getattr(pkg, name) == value, name
        assert "pub const KSCHED_%s: u32 = 0x%x;" % (name, value) in sys_rs, name
        assert '("KSCHED_%s", KSCHED_%s as i64)' % (name, name) in sys_rs, name
        assert bin(value).count("1") == 1
    # the set: spelled once from the three flags, everywhere
    assert re.search(r"#define\s+KSCHED_COMBINE_ANY\s+\(KSCHED_COMBINE_AND \| KSCHED_COMBINE_OR \| KSCHED_COMBINE_ANDNOT\)", text)
    assert _lib.COMBINE_ANY == pkg.COMBINE_ANY == _marshal.COMBINE == 0xE00
    assert "pub const KSCHED_COMBINE_ANY: u32 = KSCHED_COMBINE_AND | KSCHED_COMBINE_OR | KSCHED_COMBINE_ANDNOT;" in sys_rs
    assert '("KSCHED_COMBINE_ANY", KSCHED_COMBINE_ANY as i64)' in sys_rs


def test_the_flags_are_disjoint_from_every_other_eval_flag_and_0x1000_is_none_of_them(built):
    text = open(HEADER).read()
    from kube_scheduler_rs_reference_amd import _lib
    others = [int(v, 16) for v in re.findall(r"#define\s+KSCHED_(?:%s)\s+(0x[0-9a-fA-F]+)u" % "|".join(OTHER_FLAGS), text)]
    assert len(others) == len(OTHER_FLAGS) and all(not (v & 0xE00) for v in others)
    for name in OTHER_FLAGS:
        assert not (getattr(_lib, name) & _lib.COMBINE_ANY), name
    assert not (_lib.PICK_ANY & _lib.COMBINE_ANY)
    assert not (0x1000 & _lib.COMBINE_ANY) and 0x1000 not in VALUES.values()
    assert not re.search(r"#define\s+KSCHED_\w+\s+0x1000u\b", text), "0x1000 stays the value callers probe with as unknown"


def test_the_abi_is_still_7_and_no_function_was_added(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_COMBINE_AND\b", text)
    assert re.search(r"#define\s+KSCHED_ABI_VERSION\s+7u", text)
    assert len(FUNCTIONS) == 57 and header_functions() == set(FUNCTIONS)
    from kube_scheduler_rs_reference_amd import _lib
    assert _lib.ABI_VERSION == 7 and set(_lib.SYMBOLS) == set(FUNCTIONS)
    assert _lib.load().ksched_abi_version() == 7
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in open(SYS_RS).read()


@pytest.mark.parametrize("name", sorted(VALUES))
def test_null_ctx_is_an_error_not_a_crash(built, name):
    import numpy as np
    from kube_scheduler_rs_reference_amd import FIT, PICK_UNIFORM, _lib
    flag = VALUES[name]
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
