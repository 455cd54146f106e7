"""KSCHED_PICK_UNIFORM at the C boundary, without a GPU: the constant in the header, the Python binding and the Rust binding with one
value; the ABI version and the set of declared functions unchanged (the flag is detected by its constant and its behaviour); a NULL ctx
refused with KSCHED_E_INVAL before anything touches a device."""
import ctypes as C
import os
import re

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ksched.h")
SYS_RS = os.path.join(ROOT, "rust", "src", "ksched_sys.rs")

# every function include/ksched.h declared before the flag existed: the flag adds none
FUNCTIONS = """ksched_create ksched_destroy ksched_abi_version ksched_device_count ksched_strerror ksched_last_error ksched_mask_words
ksched_set_option ksched_set_nodes ksched_update_nodes ksched_update_node_labels ksched_apply_bindings_device ksched_read_nodes
ksched_forget_stream ksched_num_nodes ksched_num_keys ksched_eval ksched_shard_bounds ksched_eval_begin ksched_gather_buffer
ksched_eval_end ksched_eval_device ksched_eval_device_pitched ksched_mask_pitch ksched_mask_alloc ksched_mask_free
ksched_mask_probe_report ksched_pick_device ksched_pick ksched_pipe_create ksched_pipe_destroy ksched_pipe_submit ksched_pipe_wait
ksched_pipe_wait_mask ksched_pipe_stream ksched_pipe_slot_stream ksched_reason ksched_explain ksched_summarize_device ksched_summarize
ksched_comm_unique_id ksched_comm_create ksched_comm_create_local ksched_comm_destroy ksched_comm_rank ksched_comm_size
ksched_allgather_bindings ksched_allgather_bindings_local ksched_comm_last_error ksched_apply_bindings_sharded
ksched_apply_bindings_sharded_local ksched_kernel_time_ms ksched_kernel_time_samples ksched_trace_read ksched_index_checksum
ksched_last_kernel ksched_last_pick""".split()


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(ksched_\w+)\s*\(([^;{]*?)\)\s*;", text)}


def test_the_constant_is_0x40_in_the_header_the_python_binding_and_the_rust_binding(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_PICK_UNIFORM\s+0x40u\b", text)
    from kube_scheduler_rs_reference_amd import PICK_UNIFORM, _lib
    assert _lib.PICK_UNIFORM == 0x40 and PICK_UNIFORM == 0x40
    sys_rs = open(SYS_RS).read()
    assert "pub const KSCHED_PICK_UNIFORM: u32 = 0x40;" in sys_rs
    assert '("KSCHED_PICK_UNIFORM", KSCHED_PICK_UNIFORM as i64)' in sys_rs
    # one bit, and none that another flag of ksched_eval* uses
    others = [int(v, 16) for v in re.findall(r"#define\s+KSCHED_(?:FIT|SEL|TAINT|PICK_SAMPLED|PICK_BESTFIT|WANT_FIT_MASK)\s+(0x[0-9a-fA-F]+)u", text)]
    assert len(others) == 6 and all(not (v & 0x40) for v in others)


def test_the_abi_is_still_7_and_no_function_was_added(built):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KSCHED_ABI_VERSION\s+7u", text)
    assert header_functions() == set(FUNCTIONS)
    from kube_scheduler_rs_reference_amd import _lib
    assert _lib.ABI_VERSION == 7 and set(_lib.SYMBOLS) == set(FUNCTIONS)
    assert _lib.load().ksched_abi_version() == 7
    assert "pub const KSCHED_ABI_VERSION: u32 = 7;" in open(SYS_RS).read()


def test_null_ctx_is_an_error_not_a_crash(built):
    import numpy as np
    from kube_scheduler_rs_reference_amd import FIT, PICK_UNIFORM, _lib
    lib = _lib.load()
    cpu = np.zeros(4, np.int64)
    smp = np.zeros((4, 1), np.uint32)
    mask = np.zeros((4, 2), np.uint64)
    out = np.full(4, 7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.ksched_eval(None, 4, p(cpu), p(cpu), None, None, p(smp), 1, FIT | PICK_UNIFORM, None, None, p(out)) == _lib.E_INVAL
    assert lib.ksched_eval(None, 0, None, None, None, None, None, 0, PICK_UNIFORM, None, None, None) == _lib.E_INVAL
    assert lib.ksched_pick(None, 4, p(mask), None, p(smp), 1, PICK_UNIFORM, p(out)) == _lib.E_INVAL
    assert lib.ksched_pick_device(None, 4, None, 2, None, None, 1, PICK_UNIFORM, None, None) == _lib.E_INVAL
    assert (out == 7).all()
