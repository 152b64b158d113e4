"""GPU: the four HIP VAE objects launch what they launched, write the bits they wrote and hold the bytes they held before their forward
steps were shared and the GroupNorm hand-off / zero-border invariants became explicit.

tools/vae_bits.py wraps the library handle in a recorder and runs a fixed list of decodes and encodes through the public surface of
regione_amd/vae.py and regione_amd/qwen_vae.py (every switch both ways, square / wide / odd sizes, both tile geometries, the reuse walk of
tests/test_gpu_vae_reuse.py with the device bytes the objects hold at its end) on seeded weights and inputs; per case it prints the number
of launches, a sha256 of the launch record (entry names and every scalar argument) and a sha256 of the output.
tests/golden/vae_bits_parent.txt is that listing from the PARENT commit on an MI355X.  Every line has to be equal: there is no tolerance."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vae_bits_parent.txt")


@pytest.mark.gpu
def test_every_line_equals_the_parent_commits():
    """The tool runs as a process of its own, as it did for the golden listing: its last lines are differences of an allocator statistic,
    and what a long-lived process allocated and freed before moves them (the same tree printed 351246336 and 200378368 bytes for the KL and
    Qwen walks behind 1400 other tests, 352700416 and 199645696 alone).  Nothing else of the listing depends on the process."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vae_bits.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-4000:]
    want = [l.rstrip("\n") for l in open(GOLDEN) if not l.startswith("#")]
    got = [l for l in run.stdout.splitlines() if not l.startswith("#")]
    assert len(want) == 159 and got == want
