"""KSCHED_PICK_PACK at the C boundary, without a GPU: the constant in the header, the Python binding, the package and the Rust binding
with one value; one bit that no other flag of ksched_eval* uses; the ABI version and the set of declared functions unchanged (the flag is
detected by its constant and by KSCHED_E_INVAL from an older library); a NULL ctx refused with KSCHED_E_INVAL before anything touches a
device, outputs untouched."""
import ctypes as C
import re

from tests.test_uniform_abi import FUNCTIONS, HEADER, SYS_RS, header_functions


def test_the_constant_is_0x100_in_the_header_the_python_binding_and_the_rust_binding(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_PICK_PACK\s+0x100u\b", text)
    import kube_scheduler_rs_reference_amd as pkg
    from kube_scheduler_rs_reference_amd import _lib
    assert _lib.PICK_PACK == 0x100 and pkg.PICK_PACK == 0x100
    sys_rs = open(SYS_RS).read()
    assert "pub const KSCHED_PICK_PACK: u32 = 0x100;" in sys_rs
    assert '("KSCHED_PICK_PACK", KSCHED_PICK_PACK as i64)' in sys_rs
    # one bit, and none that another flag of ksched_eval* uses
    others = [int(v, 16) for v in
              re.findall(r"#define\s+KSCHED_(?:FIT|SEL|TAINT|PICK_SAMPLED|PICK_BESTFIT|WANT_FIT_MASK|PICK_UNIFORM|PICK_SPREAD)\s+(0x[0-9a-fA-F]+)u", text)]
    assert len(others) == 8 and all(not (v & 0x100) for v in others)
    assert bin(0x100).count("1") == 1
    for name in ("FIT", "SEL", "TAINT", "PICK_SAMPLED", "PICK_BESTFIT", "WANT_FIT_MASK", "PICK_UNIFORM", "PICK_SPREAD"):
        assert not (getattr(_lib, name) & 0x100), name
    from kube_scheduler_rs_reference_amd import _marshal, evaluator
    assert _marshal.DRAWS & 0x100 and evaluator._PICKS & 0x100


def test_the_abi_is_still_7_and_no_function_was_added(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_PICK_PACK\b", text)
    assert re.search(r"#define\s+KSCHED_ABI_VERSION\s+7u", text)
    assert len(FUNCTIONS) == 57 and header_functions() == set(FUNCTIONS)
    from kube_scheduler_rs_reference_amd import _lib
    assert _lib.ABI_VERSION == 7 and set(_lib.SYMBOLS) == set(FUNCTIONS)
    assert _lib.load().ksched_abi_version() == 7
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in open(SYS_RS).read()


def test_null_ctx_is_an_error_not_a_crash(built):
    import numpy as np
    from kube_scheduler_rs_reference_amd import FIT, PICK_PACK, _lib
    lib = _lib.load()
    cpu = np.zeros(4, np.int64)
    smp = np.zeros((4, 3), np.uint32)
    mask = np.zeros((4, 2), np.uint64)
    out = np.full(4, 7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.ksched_eval(None, 4, p(cpu), p(cpu), None, None, p(smp), 3, FIT | PICK_PACK, None, None, p(out)) == _lib.E_INVAL
    assert lib.ksched_eval(None, 0, None, None, None, None, None, 0, PICK_PACK, None, None, None) == _lib.E_INVAL
    assert lib.ksched_pick(None, 4, p(mask), None, p(smp), 3, PICK_PACK, p(out)) == _lib.E_INVAL
    assert lib.ksched_pick_device(None, 4, None, 2, None, None, 3, PICK_PACK, None, None) == _lib.E_INVAL
    assert (out == 7).all()
