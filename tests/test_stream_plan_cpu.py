"""The host-side batch plans (kaldi-aslp_amd/nnet/stream-batch-plan.h: delay clamp, skip offsets, the rewind by the right context, streams
that never received an utterance) against the loops they restate, in a stand-alone program built with -fsanitize=address,undefined.
No GPU and nothing loaded into this process: the program is compiled and run as a child."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_plans_under_sanitizers():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "kaldi-aslp_amd"), "plancheck"], capture_output=True, timeout=600)
    out = p.stdout.decode() + p.stderr.decode()
    assert p.returncode == 0, out[-3000:]
    assert "stream_plan_check: ok" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out
