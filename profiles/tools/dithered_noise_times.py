"""What the blue-noise dithered sampling table costs and does (include/vkr_noise_table.h generate_dithered_noise_table).

    python profiles/tools/dithered_noise_times.py times [out.json]     the default call six times with HIP events on the
        device's stream around it (allocation, kernels, read-back), 2^16 rounds at five resolutions, and the numpy
        restatement of 64 rounds of the default table on this host
    python profiles/tools/dithered_noise_times.py curve [out.json]     the mean distance between the values of 4-neighbours
        (noise_tables.dithered_neighbour_distance) of the default table after 2^k rounds, k = 0 ... 20, two seeds
    python profiles/tools/dithered_noise_times.py variance [out.json]  config 3 of the test-suite's scene at 256x256 with
        shadow rays: the mean sample variance of 64 frames (convergence.measure) with the white, blue, owen and dithered
        tables (the last at its default round count and at six smaller ones), and the RMSE of 16 single frames against the
        mean of 4096 white-noise frames, plain and after a Gaussian blur of sigma = 2 pixels
    rocprofv3 --kernel-trace --stats --output-format csv -d out/trace -o t -- python profiles/tools/dithered_noise_times.py times"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vulkan_renderer_amd import capi, convergence, renderer, synthetic  # noqa: E402
from vulkan_renderer_amd import noise_tables as nt  # noqa: E402

TYPE = "blue_noise_dithered"


def host_table(r):
    n = r.app.noise_table.resolution
    return np.ctypeslib.as_array(r.app.noise_table.host_data, (n.depth, n.height, n.width, 4)).copy()


def times():
    hip = C.CDLL("libamdhip64.so")
    r = renderer.Renderer()
    stream = C.c_void_p(r.app.device.stream)
    start, stop = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0

    def call(resolution, seed, rounds):
        r.lib.destroy_noise_table(C.byref(r.app.noise_table), C.byref(r.app.device))
        r.sync()
        assert hip.hipEventRecord(start, stream) == 0
        assert r.lib.generate_dithered_noise_table(C.byref(r.app.noise_table), C.byref(r.app.device), capi.Extent3D(*resolution), seed, rounds) == 0
        assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
        return ms.value

    out = {}
    resolution = nt.default_resolution(TYPE)
    rounds = r.lib.get_default_dithered_round_count(capi.Extent3D(*resolution))
    all_ms = [call(resolution, i, rounds) for i in range(6)]
    out["default"] = {"resolution": resolution, "rounds": rounds, "hip_event_ms": sorted(all_ms[1:])[2], "hip_event_ms_all": all_ms}
    print("default", json.dumps(out["default"]), flush=True)
    out["per_round"] = []
    for resolution in ((16, 32, 1), (32, 32, 1), (64, 64, 1), (128, 128, 1), (128, 128, 64), (256, 128, 1)):
        none = sorted(call(resolution, 0, 0) for _ in range(3))[1]
        some = sorted(call(resolution, 0, 1 << 16) for _ in range(3))[1]
        row = {"resolution": resolution, "ms_0_rounds": none, "ms_65536_rounds": some, "us_per_round": (some - none) * 1.0e3 / (1 << 16)}
        out["per_round"].append(row)
        print(json.dumps(row), flush=True)
    r.close()
    t0 = time.perf_counter()
    packed = nt.dithered_initial(128, 128, 0, 0)
    t1 = time.perf_counter()
    nt.dithered_rounds(packed, 128, 128, 0, 0, 0, 64)
    out["numpy"] = {"initial_seconds": t1 - t0, "seconds_per_round_and_array": (time.perf_counter() - t1) / 64}
    print("numpy", json.dumps(out["numpy"]), flush=True)
    return out


def curve():
    r = renderer.Renderer()
    out = []
    for seed in (0, 5):
        for rounds in [0] + [1 << k for k in range(21)]:
            r.generate_noise_table(TYPE, None, seed, rounds)
            table = host_table(r)
            arrays = [table[0, :, :, 2 * a:2 * a + 2] for a in range(2)]
            row = {"seed": seed, "rounds": rounds, "neighbour_distance": float(np.mean([nt.dithered_neighbour_distance(a) for a in arrays])),
                   "low_frequency_share": float(np.mean([nt.dithered_low_frequency_share(a) for a in arrays]))}
            out.append(row)
            print(json.dumps(row), flush=True)
    r.close()
    return out


def blurred(image, sigma):
    """Gaussian blur of (H, W, C) with wrap-around, by FFT"""
    height, width, _ = image.shape
    fy, fx = np.fft.fftfreq(height)[:, None], np.fft.fftfreq(width)[None, :]
    response = np.exp(-2.0 * np.pi ** 2 * sigma ** 2 * (fx ** 2 + fy ** 2))
    return np.fft.ifft2(np.fft.fft2(image, axes=(0, 1)) * response[..., None], axes=(0, 1)).real


def variance():
    out = []
    with tempfile.TemporaryDirectory() as d:
        dataset = synthetic.write_dataset(d, grid=64, box_count=24, seed=1234, ltc_resolution=16, fresnel_count=8)
        for sample_count in (2, 8):
            r = renderer.Renderer(frames_in_flight=3, arithmetic="libm")
            renderer.setup_config(r, 3, dataset, width=256, height=256, animate_noise=True, trace_shadow_rays=True, acceleration_structure="sah_device", sample_count=sample_count)
            r.create_targets()
            r.create_pass()
            r.render_visibility()
            reference = convergence.measure(r, 4096, seed=500000, return_mean=True)["mean"][..., :3].astype(np.float64)
            for noise, rounds in (("white", None), ("blue", None), ("owen", None), (TYPE, None), (TYPE, 0), (TYPE, 1 << 8), (TYPE, 1 << 10), (TYPE, 1 << 12), (TYPE, 1 << 14), (TYPE, 1 << 16)):
                if noise != "white":
                    r.generate_noise_table(noise, seed=0, rounds=rounds)
                row = {"sample_count": sample_count, "noise": noise, "rounds": rounds, "mean_variance": convergence.measure(r, 64, seed=1000)["mean_variance"]}
                plain, smooth = [], []
                for frame in range(16):
                    r.finish_frames()
                    r.app.noise_table.random_seed = 2000 + frame
                    r.render()
                    error = r.read_radiance()[..., :3].astype(np.float64) - reference
                    plain.append(float(np.sqrt((error ** 2).mean())))
                    smooth.append(float(np.sqrt((blurred(error, 2.0) ** 2).mean())))
                row["rmse"], row["rmse_blurred"] = float(np.mean(plain)), float(np.mean(smooth))
                out.append(row)
                print(json.dumps(row), flush=True)
            r.close()
    return out


if __name__ == "__main__":
    result = {"times": times, "curve": curve, "variance": variance}[sys.argv[1]]()
    if len(sys.argv) > 2:
        json.dump(result, open(sys.argv[2], "w"), indent=1)
