"""bench.py at a small shape on the GPU: a plain run prints the headline line only and --dump-outputs writes what the last timed
step computed; --full adds the measurements beyond the headline, and its timed path computes the same arrays from the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--frames", "8", "--framesize", "128", "--fft_len", "256"]
NAMES = {"loss", "attention_frames", "x_stft", "y_stft", "pred_audio", "pred_video", "fused", "params"}


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_full_adds_the_rest(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert d["steps"] == 3 and d["n_gpus"] == 1 and d["unit"] == "clips/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["value"] == pytest.approx(2 * 1e3 / d["ms_per_step"], rel=1e-3)
    assert not {"roofline", "stages", "kernel_ms_per_step", "cpu_baseline", "ms_per_step_one_stream"} & d.keys()
    files = sorted((tmp_path / "plain").glob("*.npy"))
    assert {p.stem for p in files} == NAMES
    assert sum(p.stat().st_size for p in files) <= 64 << 20
    plain = {p.stem: np.load(p) for p in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in plain.values())
    assert plain["loss"].shape == (3,) and plain["loss"][2] == pytest.approx(d["config"]["loss"], rel=1e-6)
    assert plain["attention_frames"].shape == (2, 1, 8, 128, 128)

    f = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert f["steps"] == 3 and {"roofline", "stages", "kernel_ms_per_step", "ms_per_step_one_stream"} <= f.keys()
    full = {n: np.load(tmp_path / "full" / f"{n}.npy") for n in NAMES}
    for n in ("attention_frames", "x_stft", "y_stft"):         # the ViT and the STFT accumulate without atomics: bit-identical
        assert np.array_equal(plain[n], full[n]), n
    for n in ("loss", "pred_audio", "pred_video", "fused", "params"):   # the split-K Linear layers sum by f32 atomics
        np.testing.assert_allclose(plain[n], full[n], rtol=1e-3, atol=1e-4, err_msg=n)
