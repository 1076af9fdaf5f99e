"""bench.py --dump-outputs DIR: the frame the timed path computed in its last step, written as DIR/<name>.npy so that two
builds can be compared output for output; and the plain run (no --full), which times the steps and prints the line without
measuring anything beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs():
    sys.path.insert(0, ROOT)
    from vulkan_renderer_amd.bench import outputs
    return outputs


def test_outputs_under_the_limit_are_written_whole(tmp_path):
    outputs = _outputs()
    frame = np.random.default_rng(1).random((54, 96, 4), dtype=np.float32)
    assert outputs.write_outputs(str(tmp_path), {"radiance": frame}) == ["radiance"]
    back = np.load(tmp_path / "radiance.npy")
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), frame.view(np.uint32))
    assert sorted(os.listdir(tmp_path)) == ["radiance.npy"]


def test_outputs_over_the_limit_are_a_fixed_seeded_sample_of_whole_pixels(tmp_path):
    """a 3840x2160 RGBA32F frame (133 MB) does not fit 64 MB: the same pixels are sampled in every run, and their indices are
    written beside them"""
    outputs = _outputs()
    frame = np.arange(120 * 200 * 4, dtype=np.float32).reshape(120, 200, 4)
    limit = frame.nbytes // 4
    for run in ("a", "b"):
        assert outputs.write_outputs(str(tmp_path / run), {"radiance": frame}, limit=limit) == ["radiance_pixel_index", "radiance"]
    sample, index = np.load(tmp_path / "a" / "radiance.npy"), np.load(tmp_path / "a" / "radiance_pixel_index.npy")
    assert sample.dtype == np.float32 and index.dtype == np.float64
    assert sample.nbytes + index.nbytes <= limit and len(sample) > 0.9 * limit / (16 + 8)
    assert np.all(np.diff(index) > 0) and index[-1] < 120 * 200
    assert np.array_equal(sample, frame.reshape(-1, 4)[index.astype(np.int64)])
    assert np.array_equal(sample, np.load(tmp_path / "b" / "radiance.npy"))
    assert np.array_equal(index, np.load(tmp_path / "b" / "radiance_pixel_index.npy"))


def test_outputs_are_floating_point(tmp_path):
    outputs = _outputs()
    with pytest.raises(AssertionError):
        outputs.write_outputs(str(tmp_path), {"encoded": np.zeros((4, 4, 4), np.uint8)})


def test_the_plain_run_and_the_full_run_are_both_offered():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert done.returncode == 0, done.stderr[-1000:]
    assert "--full" in done.stdout and "--dump-outputs" in done.stdout


@pytest.mark.gpu
def test_a_plain_run_times_the_steps_it_is_given_and_dumps_the_frame_of_the_last_one(tmp_path, big_dataset):
    """A plain run of BASELINE config 2: one line with the headline keys and the requested steps, nothing measured beside it;
    the dumped frame is the frame an independent render of the same workload (the benchmark's scene, libm arithmetic) gives,
    bit for bit."""
    from vulkan_renderer_amd import renderer
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "VKR_BENCH_SELF_LAUNCHED")}
    out = tmp_path / "outputs"
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--steps", "30", "--warmup", "3", "--prewarm-frames", "8",
                           "--prewarm-seconds", "0.2", "--dump-outputs", str(out)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-1500:] + done.stderr[-1500:]
    lines = [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 30 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1920 * 1080 * 1 / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * line["value"]
    assert line["roofline"] is None and line["details"] is None
    assert not set(("cpu_baseline", "parity", "secondary", "extra_workloads", "other_modes", "latency_ms")) & set(line)
    assert sorted(os.listdir(out)) == ["radiance.npy"]
    dumped = np.load(out / "radiance.npy")
    assert dumped.dtype == np.float32 and dumped.shape == (1080, 1920, 4)

    r = renderer.Renderer(arithmetic="libm", frames_in_flight=1)
    renderer.setup_config(r, 2, big_dataset, width=1920, height=1080, acceleration_structure="sah_device")
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    frame = r.read_radiance()
    r.close()
    assert not np.isnan(dumped).any()
    assert np.array_equal(dumped.view(np.uint32), frame.view(np.uint32)), int((dumped.view(np.uint32) != frame.view(np.uint32)).any(axis=-1).sum())
