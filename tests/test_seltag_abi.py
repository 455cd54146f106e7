"""KSCHED_SELOP_TAGGED and KSCHED_SELTAG_* at the C boundary, without a GPU: the constants in the header, the Python binding, the package
and the Rust binding with one value each; the flag a single bit outside the predicate, pick and output flags (0x1FF), the combine ops
(0xE00), the soft modifier (0x2000), the operator flags (0x1C000, whose spelled #define does not take it in) and the two values callers probe
with as unknown (0x1000, 0x20000); the ABI version and the set of declared functions unchanged (the flag is detected by its constant and by
KSCHED_E_INVAL from an older library); a NULL ctx refused with KSCHED_E_INVAL before anything touches a device, outputs untouched."""
import ctypes as C
import re

from tests.test_uniform_abi import FUNCTIONS, HEADER, SYS_RS, header_functions

TAGGED = 0x40000
# name -> (value, how the header writes it, how the Rust binding writes it)
VALUES = {
    "SELOP_TAGGED": (0x40000, "0x40000u", "0x40000"),
    "SELTAG_SHIFT": (29, "29u", "29"),
    "SELTAG_ID_MASK": (0x1FFFFFFF, "0x1FFFFFFFu", "0x1FFFFFFF"),
    "SELTAG_EQ": (0, "0u", "0"),
    "SELTAG_NE": (1, "1u", "1"),
    "SELTAG_EXISTS": (2, "2u", "2"),
    "SELTAG_ABSENT": (3, "3u", "3"),
    "SELTAG_GT": (4, "4u", "4"),
    "SELTAG_LT": (5, "5u", "5"),
}


def test_the_constants_have_one_value_in_the_header_the_python_binding_and_the_rust_binding(built):
    text = open(HEADER).read()
    sys_rs = open(SYS_RS).read()
    import kube_scheduler_rs_reference_amd as pkg
    from kube_scheduler_rs_reference_amd import _lib
    for name, (value, c_text, rs_text) in VALUES.items():
        assert len(re.findall(r"#define\s+KSCHED_%s\s+%s(?!\w)" % (name, c_text), text)) == 1, name
        assert len(re.findall(r"#define\s+KSCHED_%s\b" % name, text)) == 1, name
        assert getattr(_lib, name) == value and getattr(pkg, name) == value, name
        assert "pub const KSCHED_%s: u32 = %s;" % (name, rs_text) in sys_rs, name
        assert '("KSCHED_%s", KSCHED_%s as i64)' % (name, name) in sys_rs, name
    assert _lib.SELTAG_ID_MASK == (1 << _lib.SELTAG_SHIFT) - 1 and _lib.SEL_NEVER >> _lib.SELTAG_SHIFT == 7
    assert callable(pkg.seltag)


def test_the_flag_is_a_single_bit_outside_every_other_flag_set_and_the_probed_values(built):
    text = open(HEADER).read()
    from kube_scheduler_rs_reference_amd import _lib
    others = _lib.FIT | _lib.SEL | _lib.TAINT | _lib.PICK_ANY | _lib.WANT_FIT_MASK
    assert others == 0x1FF and _lib.COMBINE_ANY == 0xE00 and _lib.COMBINE_SOFT == 0x2000 and _lib.SELOP_ANY == 0x1C000
    assert bin(TAGGED).count("1") == 1
    assert not TAGGED & (0x1FF | 0xE00 | 0x2000 | 0x1C000 | 0x1000 | 0x20000)
    # not a member of KSCHED_SELOP_ANY: its #define stays spelled from exactly the three operators
    assert re.search(r"#define\s+KSCHED_SELOP_ANY\s+\(KSCHED_SELOP_EXISTS \| KSCHED_SELOP_GT \| KSCHED_SELOP_LT\)", text)
    for probe in ("0x1000u", "0x20000u"):
        assert not re.search(r"#define\s+KSCHED_\w+\s+%s(?!\w)" % probe, text), probe + " stays a value callers probe with as unknown"
    # the flag lists other tests read off the header do not take the new names for the old ones
    old = re.findall(r"#define\s+KSCHED_(?:FIT|SEL|TAINT|PICK_\w+|WANT_FIT_MASK|COMBINE_AND|COMBINE_OR|COMBINE_ANDNOT|COMBINE_SOFT)\s+(0x[0-9a-fA-F]+)u", text)
    assert len(old) == 13 and all(not (int(v, 16) & TAGGED) for v in old)


def test_the_abi_is_still_7_and_no_function_was_added(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_SELOP_TAGGED\b", text)
    assert re.search(r"#define\s+KSCHED_ABI_VERSION\s+7u", text)
    assert len(FUNCTIONS) == 57 and header_functions() == set(FUNCTIONS)
    from kube_scheduler_rs_reference_amd import _lib
    assert _lib.ABI_VERSION == 7 and set(_lib.SYMBOLS) == set(FUNCTIONS) and len(_lib.SYMBOLS) == 57
    assert _lib.load().ksched_abi_version() == 7
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in open(SYS_RS).read()


def test_null_ctx_is_an_error_not_a_crash(built):
    import numpy as np
    from kube_scheduler_rs_reference_amd import COMBINE_AND, PICK_UNIFORM, SEL, SELOP_TAGGED, _lib
    flag = SELOP_TAGGED
    lib = _lib.load()
    cpu = np.zeros(4, np.int64)
    sel = np.ones((1, 4), np.uint32)
    smp = np.zeros((4, 3), np.uint32)
    mask = np.full((4, 2), 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = np.full(4, 7, np.int32)
    table = np.full((4, _lib.SUMMARY_WORDS), 7, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.ksched_eval_device(None, 4, p(cpu), p(cpu), p(sel), None, None, 0, SEL | flag, p(mask), None, None, None) == _lib.E_INVAL
    assert lib.ksched_eval_device_pitched(None, 4, p(cpu), p(cpu), p(sel), None, p(smp), 3, SEL | flag | COMBINE_AND | PICK_UNIFORM, p(mask), None, p(out), 2, None) == _lib.E_INVAL
    assert lib.ksched_eval(None, 4, p(cpu), p(cpu), p(sel), None, None, 0, SEL | flag, p(mask), None, None) == _lib.E_INVAL
    dev_b, stream = C.c_void_p(), C.c_void_p()
    assert lib.ksched_eval_begin(None, 4, p(cpu), p(cpu), p(sel), 4, None, None, 0, SEL | flag, p(mask), None, 4, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
    assert not dev_b.value and not stream.value
    assert lib.ksched_pick(None, 4, p(mask), None, p(smp), 3, PICK_UNIFORM | flag, p(out)) == _lib.E_INVAL
    assert lib.ksched_pick_device(None, 4, None, 2, None, None, 3, PICK_UNIFORM | flag, None, None) == _lib.E_INVAL
    assert lib.ksched_pipe_submit(None, 0, 4, p(cpu), p(cpu), p(sel), None, p(smp), 3, SEL | flag | PICK_UNIFORM, p(mask), 2, p(out)) == _lib.E_INVAL
    assert lib.ksched_summarize(None, 4, p(cpu), p(cpu), p(sel), None, SEL | flag, p(table)) == _lib.E_INVAL
    assert lib.ksched_explain(None, 4, p(cpu), p(cpu), p(sel), None, 1, p(smp), p(smp), SEL | flag, p(out)) == _lib.E_INVAL
    assert (out == 7).all() and (mask == 0x5A5A5A5A5A5A5A5A).all() and (table == 7).all()
