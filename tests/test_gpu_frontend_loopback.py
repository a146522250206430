"""One small run of the front-end arms of tools/loopback_per.py (NUMERICS.md rule 32): 2048 frames, one SNR, three arms."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loopback_arms_off_dc_dc_iq(tmp_path):
    """a DC offset 10 dB above the noise: the receiver without a front end delivers fewer good frames than the one with the DC
    stage -- the ordering of scene (a) of tests/frontend_scene.py, nothing more; the figures themselves are records
    (profiles/loopback_frontend.json)"""
    out = tmp_path / "loopback_frontend.json"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "loopback_per.py"), "--frames", "2048", "--snr", "30", "--dc-db", "10",
                           "--frontend", "off", "dc", "dc+iq", "--out", str(out)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    res = json.loads(out.read_text())
    assert len(res["points"]) == 1
    arms = res["points"][0]["arms"]
    assert sorted(arms) == ["dc", "dc+iq", "off"]
    for arm in arms.values():
        assert arm["counts"]["frames"] == 2048 and 0.0 <= arm["fer"] <= 1.0
    print({k: (v["fer"], v["fer_soft"]) for k, v in arms.items()})
    assert arms["off"]["counts"]["frames_psdu_ok"] < arms["dc"]["counts"]["frames_psdu_ok"]
