"""The plain-C host's `widen` mode (examples/c_host/net_host.c): net_g19's set, the channel-selected
19 x 480 network the example links, widened to the 64 rows of the whole cap through net_blob_widen
from C, and the widened set's logits on u[64][T] held to the original's on the gathered rows."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples", "c_host")
pytestmark = pytest.mark.gpu


def test_c_host_widens_net_g19_to_64_rows(gpu, tmp_path):
    sys.path.insert(0, EX)
    import make_nets

    subprocess.run(["make", "-s", "-C", EX], check=True)
    blob = tmp_path / "g19.blob"
    blob.write_bytes(make_nets.param_set("net_g19").to_blob())
    r = subprocess.run([os.path.join(EX, "net_host"), "widen", str(blob), "64", "24"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "widened 19 -> 64 rows" in r.stdout and "0 of 24 trials differ" in r.stdout and "ok" in r.stdout
    # a montage narrower than the network is refused by the library, and the host says so
    r = subprocess.run([os.path.join(EX, "net_host"), "widen", str(blob), "16", "4"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "net_blob_widen: invalid argument" in r.stderr
