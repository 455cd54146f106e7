"""The ctx's stream ordering (csrc/stream_order.hpp) checked on the host, no GPU: which stream carries a snapshot change, which streams
wait for which event before an evaluation, a change, an apply or a use of ctx-owned scratch is enqueued, and what is recorded for that --
over a happens-before model of every sequence of up to five calls (evaluations on the own stream and on two caller streams, with and
without scratch, set / update, applies from four streams, a best-fit rebuild in front of an evaluation, a stream forgotten, a stream
destroyed without notice, KSCHED_OPT_SNAPSHOT_STREAM switched), call for call against the rules as they were before the header, the
steady states written out and the hot path's allocations counted: tests/cpp/stream_order_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "stream_order_tests")


def test_stream_order_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/stream_order_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
