"""ksched_apply_bindings_device / ksched_read_nodes (ABI 7) at the C boundary, without a GPU: exported, declared with the
issue's constants, NULL contexts refused without a crash, and the version number moved with the surface."""
import os
import re

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ksched.h")

EXPECTED = {
    "APPLY_FIRST_PER_NODE": 0x01,
    "APPLY_RELEASE": 0x02,
    "APPLY_APPLIED": 0,
    "APPLY_UNBOUND": 1,
    "APPLY_NOT_OK": 2,
    "APPLY_DEFERRED": 3,
    "APPLY_OVERFLOW": 4,
    "APPLY_BAD_NODE": 5,
}


def header_defines():
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+KSCHED_([A-Z_0-9]+)\s+\(?(-?(?:0x)?[0-9A-Fa-f]+)u?\)?", text)}


def test_header_declares_the_apply_constants():
    defs = header_defines()
    for k, v in EXPECTED.items():
        assert defs.get(k) == v, k
    assert defs["ABI_VERSION"] == 7


def test_python_binding_carries_the_apply_constants(built):
    from kube_scheduler_rs_reference_amd import _lib
    for k, v in EXPECTED.items():
        assert getattr(_lib, k) == v, k
    assert _lib.ABI_VERSION == 7


def test_library_exports_apply_and_read_nodes(built):
    from kube_scheduler_rs_reference_amd import _lib
    lib = _lib.load()
    assert lib.ksched_abi_version() == 7
    for name in ("ksched_apply_bindings_device", "ksched_read_nodes"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS


def test_null_ctx_is_an_error_not_a_crash(built):
    from kube_scheduler_rs_reference_amd import _lib
    lib = _lib.load()
    assert lib.ksched_apply_bindings_device(None, 0, None, None, None, None, 0, None, None) == _lib.E_INVAL
    assert lib.ksched_apply_bindings_device(None, 4, None, None, None, None, _lib.APPLY_FIRST_PER_NODE, None, None) == _lib.E_INVAL
    assert lib.ksched_read_nodes(None, 0, 0, None, None) == _lib.E_INVAL
    assert lib.ksched_read_nodes(None, 0, 8, None, None) == _lib.E_INVAL


def test_rust_binding_declares_apply_and_read_nodes():
    sys_rs = open(os.path.join(ROOT, "rust", "src", "ksched_sys.rs")).read()
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in sys_rs
    for name in ("ksched_apply_bindings_device", "ksched_read_nodes"):
        assert f"pub fn {name}(" in sys_rs and f'("{name}", {name} as usize)' in sys_rs
    for k, v in EXPECTED.items():
        m = re.search(rf"pub const KSCHED_{k}: \w+ = (0x[0-9A-Fa-f_]+|\d+);", sys_rs)
        assert m and int(m.group(1).replace("_", ""), 0) == v, k
