"""ksched_summarize / ksched_summarize_device at the C boundary, without a GPU: exported with the documented arity, declared alike in
the header, the Python binding and the Rust binding, the ABI version unchanged (they are detected by symbol), and a NULL ctx -- with
good or bad flags, with or without pointers -- refused with KSCHED_E_INVAL before anything touches a device."""
import ctypes as C
import os
import re

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ksched.h")
SYS_RS = os.path.join(ROOT, "rust", "src", "ksched_sys.rs")
ARITY = {"ksched_summarize_device": 9, "ksched_summarize": 8}


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(ksched_\w+)\s*\(([^;{]*?)\)\s*;", text)}


def test_header_declares_both_entry_points_and_the_constant():
    fns = header_functions()
    for name, n in ARITY.items():
        assert fns.get(name) == n, name
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_SUMMARY_WORDS\s+4u", text)
    assert re.search(r"#define\s+KSCHED_ABI_VERSION\s+7u", text)
    # the table is indexed by the reason codes
    for k, v in (("OK", 0), ("NOT_ENOUGH_RESOURCES", 1), ("NODE_SELECTOR_MISMATCH", 2), ("TAINT_NOT_TOLERATED", 3)):
        assert re.search(rf"#define\s+KSCHED_REASON_{k}\s+{v}\b", text), k


def test_python_binding_declares_them(built):
    from kube_scheduler_rs_reference_amd import Evaluator, _lib
    assert _lib.SUMMARY_WORDS == 4 and _lib.ABI_VERSION == 7
    for name, n in ARITY.items():
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n and _lib.SYMBOLS[name][0] is C.c_int, name
    assert callable(Evaluator.summarize) and callable(Evaluator.summarize_device)
    from kube_scheduler_rs_reference_amd import dist
    assert callable(dist.AbiComm.summarize) and callable(dist.LocalClique.summarize)


def test_library_exports_them_and_the_abi_is_still_7(built):
    from kube_scheduler_rs_reference_amd import _lib
    lib = _lib.load()
    assert lib.ksched_abi_version() == 7
    for name in ARITY:
        assert hasattr(lib, name), name
    # the test build of the library is made of the same objects
    hooks = os.path.join(ROOT, "tests", "cpp", "hooks", "libksched_hip.so")
    assert os.path.exists(hooks)
    test_lib = C.CDLL(hooks)
    for name in ARITY:
        assert hasattr(test_lib, name), name


def test_rust_binding_declares_them():
    sys_rs = open(SYS_RS).read()
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in sys_rs
    assert re.search(r"pub const KSCHED_SUMMARY_WORDS: u32 = 4;", sys_rs)
    text = re.sub(r"//[^\n]*", "", sys_rs)
    for name, n in ARITY.items():
        m = re.search(rf"pub fn {name}\s*\(([^;]*?)\)\s*->\s*c_int;", text, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, name
        assert f'("{name}", {name} as usize)' in sys_rs


def test_null_ctx_and_bad_arguments_are_errors_not_crashes(built):
    import numpy as np
    from kube_scheduler_rs_reference_amd import FIT, SEL, TAINT, _lib
    lib = _lib.load()
    cpu = np.zeros(4, np.int64)
    out = np.zeros((4, 4), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for flags in (FIT, FIT | SEL | TAINT, 0, 0x08, 0x20 | FIT, 0xFFFFFFFF):
        # NULL ctx, with and without the required pointers, p == 0 and p > 0
        assert lib.ksched_summarize(None, 0, None, None, None, None, flags, None) == _lib.E_INVAL
        assert lib.ksched_summarize(None, 4, None, None, None, None, flags, None) == _lib.E_INVAL
        assert lib.ksched_summarize(None, 4, p(cpu), p(cpu), None, None, flags, p(out)) == _lib.E_INVAL
        assert lib.ksched_summarize_device(None, 0, None, None, None, None, flags, None, None) == _lib.E_INVAL
        assert lib.ksched_summarize_device(None, 4, None, None, None, None, flags, None, None) == _lib.E_INVAL
    assert (out == 0).all()
