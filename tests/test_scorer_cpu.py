"""CPU: Convex::BatchingScorer (ngmlr_amd/csrc/batching_scorer.{h,cpp}) -- the queue behind the device-scored interval and
inversion checks -- with a host backend in place of the device (tests/cpp/batching_scorer_test.cpp): every caller gets its own
score on 2 000 fibers and on 64 threads, park and wake pair up, shutdown with requests queued serves them, and a failed launch
throws in exactly its own callers.  A lost wake-up is a hang (timeout)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "ngmlr_amd", "batching_scorer_test")


def _build():
    res = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ngmlr_amd", "csrc"), BINARY],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


@pytest.mark.parametrize("args", [
    ["fibers", "4", "2000", "20000"],     # thousands of contexts parked on four carriers
    ["fibers", "1", "64", "3000"],        # one carrier: every park and wake on one thread
    ["threads", "64", "200"],             # plain threads: the condition-variable path
    ["shutdown", "64"],                   # the scorer goes while requests wait: they are scored first
    ["fail", "64", "100"],                # every 5th launch fails (in submit or in wait): its callers throw, nobody else
])
def test_batching_scorer(built, args):
    _build()
    res = subprocess.run([BINARY] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("ok:"), res.stdout[-1000:]
