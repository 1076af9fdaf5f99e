"""Variance and error of an estimator, measured on the device (include/vkr_frame_statistics.h).

    python -m vulkan_renderer_amd.convergence --config 3 --frames 256 --reference-frames 4096 \\
        --strategy diffuse_specular_mis diffuse_specular_separately --heuristic balance optimal_clamped

renders, for every requested combination of sampling technique, strategy, MIS heuristic, arithmetic mode and noise table
(`--noise white owen blue ...`: every type but white is generated on the device, include/vkr_noise_table.h)
and LTC table (`--ltc synthetic fitted`: `fitted` replaces the data set's placeholder fits by a table fitted on the device,
include/vkr_ltc_table.h fit_ltc_table), frames with animated noise and prints one JSON line: milliseconds per frame, the mean sample variance over pixels and
channels and the RMSE of the mean of those frames against a converged image (`--reference-frames` frames of the
configuration's own settings, from another seed).  Frames never leave the GPU: they are summed per pixel in binary64
there, and the error sums are reduced there."""
import argparse
import ctypes as C
import itertools
import json
import math
import sys
import tempfile
import time

import numpy as np

from . import noise_tables
from . import renderer as renderer_module
from . import synthetic

BATCH = 4  # frames per accumulate_frames() call; the ring holds two batches


class _DeviceTargets:
    """RGBA32F device buffers of the frame's size"""

    def __init__(self, count, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        self.pointers = []
        for _ in range(count):
            pointer = C.c_void_p()
            if self.hip.hipMalloc(C.byref(pointer), C.c_size_t(nbytes)):
                self.free()
                raise RuntimeError("out of device memory for %d targets of %d bytes" % (count, nbytes))
            self.pointers.append(pointer)

    def upload(self, index, array):
        a = np.ascontiguousarray(array, np.float32)
        if a.nbytes != self.nbytes or self.hip.hipMemcpy(self.pointers[index], C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1):
            raise RuntimeError("uploading the reference image failed")

    def download(self, index, shape):
        out = np.zeros(shape, np.float32)
        if out.nbytes != self.nbytes or self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.pointers[index], C.c_size_t(out.nbytes), 2):
            raise RuntimeError("reading the mean back failed")
        return out

    def free(self):
        for pointer in self.pointers:
            self.hip.hipFree(pointer)
        self.pointers = []


def measure(renderer, frames, reference_mean=None, seed=None, return_mean=False, mean_hdr=None, mean_png=None):
    """Renders `frames` frames with animated noise into a ring of targets and accumulates them on the device.  `renderer`
    has its targets, its pass and its visibility buffer.  reference_mean: a float32 image (height, width, 4) to take the
    RMSE against; seed: noise_table_t.random_seed of the first frame (default: wherever the sequence stands).
    Returns {"frames", "ms_per_frame", "mean_variance" (sample variance, ddof = 1, averaged over pixels and R, G, B; None for
    one frame), "rmse" (of the accumulated mean against the reference over pixels and R, G, B; None without one)} and,
    with return_mean, "mean": the accumulated mean as a float32 image.  mean_hdr: a path that gets the accumulated mean as
    a Radiance file, encoded on the device (include/vkr_hdr.h): the floats are not read back for it; "mean_hdr_bytes" is
    the size of the file.  mean_png: a path that gets the sRGB8 encoding of the accumulated mean as a PNG file, encoded on
    the device as well (include/vkr_png.h); "mean_png_bytes" is its size."""
    if frames < 1:
        raise ValueError("at least one frame")
    app = renderer.app
    extent = app.swapchain.extent
    pixels = extent.width * extent.height
    animate_before = app.render_settings.animate_noise
    app.render_settings.animate_noise = 1
    if seed is not None:
        app.noise_table.random_seed = int(seed)
    # two targets besides the ring: the variance (or mean), and the reference
    targets = _DeviceTargets(2 * BATCH + 2, 16 * pixels)
    ring, scratch, reference = targets.pointers[:2 * BATCH], targets.pointers[-2], targets.pointers[-1]
    statistics = renderer.create_statistics(pixels)
    try:
        renderer.sync()
        start = time.perf_counter()
        for first in range(0, frames, BATCH):
            count = min(BATCH, frames - first)
            batch = [ring[(first + k) % len(ring)] for k in range(count)]
            for pointer in batch:
                renderer.render(pointer)
            statistics.accumulate(batch)
        # (behind the accumulations, on the device's stream)
        statistics.resolve(scratch, None)
        renderer.sync()
        elapsed = time.perf_counter() - start
        result = {"frames": int(frames), "ms_per_frame": elapsed * 1.0e3 / frames, "mean_variance": None, "rmse": None}
        if reference_mean is not None:
            targets.upload(len(targets.pointers) - 1, reference_mean)
            result["rmse"] = math.sqrt(float(renderer.squared_error(scratch, reference, pixels).sum()) / (3 * pixels))
        if return_mean:
            result["mean"] = targets.download(len(targets.pointers) - 2, (extent.height, extent.width, 4))
        if mean_hdr:
            # (resolve() left the mean on the device's stream, which the encoder uses)
            data = renderer.encode_hdr(scratch, width=extent.width, height=extent.height)
            with open(mean_hdr, "wb") as file:
                file.write(data)
            result["mean_hdr_bytes"] = len(data)
        if mean_png:
            # the output encoding of the mean into the target of the reference, which has served its purpose
            renderer.encode_slab(scratch, reference, pixels)
            data = renderer.encode_png(reference, width=extent.width, height=extent.height)
            with open(mean_png, "wb") as file:
                file.write(data)
            result["mean_png_bytes"] = len(data)
        if frames >= 2:
            statistics.resolve(None, scratch)
            result["mean_variance"] = float(renderer.frame_sum(scratch, pixels).sum()) / (3 * pixels)
        return result
    finally:
        statistics.close()
        renderer.sync()
        targets.free()
        app.render_settings.animate_noise = animate_before


def _make_renderer(args, dataset, arithmetic, noise="white", ltc="synthetic", **overrides):
    r = renderer_module.Renderer(hip_device=args.device, frames_in_flight=args.frames_in_flight, timing_stride=1 << 30, arithmetic=arithmetic)
    try:
        renderer_module.setup_config(r, args.config, dataset, width=args.width, height=args.height, **overrides)
        if noise != "white":
            r.generate_noise_table(noise, seed=args.noise_seed)
        if ltc == "fitted":
            # (the size of the data set's table)
            r.fit_ltc_table(int(r.app.ltc_table.roughness_count), int(r.app.ltc_table.fresnel_count), args.ltc_sample_count)
        if args.roughness_factor is not None:
            r.app.render_settings.roughness_factor = args.roughness_factor
        r.create_targets()
        r.create_pass()
        r.render_visibility()
    except RuntimeError:
        r.close()
        raise
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[1, 2, 3, 4], help="BASELINE configuration (scene, lights, default settings)")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reference-frames", type=int, default=1024, help="frames of the converged image (0: no RMSE)")
    ap.add_argument("--technique", nargs="+", default=[None], choices=sorted(renderer_module.TECHNIQUE))
    ap.add_argument("--strategy", nargs="+", default=[None], choices=sorted(renderer_module.STRATEGY))
    ap.add_argument("--heuristic", nargs="+", default=[None], choices=sorted(renderer_module.MIS))
    ap.add_argument("--arithmetic", nargs="+", default=["libm"], choices=sorted(renderer_module.ARITHMETIC_MODES))
    ap.add_argument("--noise", nargs="+", default=["white"], choices=["white"] + list(noise_tables.GENERATED_TYPES), help="noise tables; all but white are generated on the device at their default resolution")
    ap.add_argument("--ltc", nargs="+", default=["synthetic"], choices=["synthetic", "fitted"], help="LTC tables: the placeholder fits of the synthetic data set, or a table fitted on the device")
    ap.add_argument("--ltc-sample-count", type=int, default=None, help="sample_count of the fit (default: that of fit_ltc_table)")
    ap.add_argument("--roughness-factor", type=float, default=None, help="render_settings.roughness_factor (below 1: a glossy variant of the configuration)")
    ap.add_argument("--noise-seed", type=int, default=0, help="generator seed of the generated tables")
    ap.add_argument("--sample-count", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--frames-in-flight", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000, help="noise seed of the first measured frame")
    ap.add_argument("--reference-seed", type=int, default=50000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mean-hdr", metavar="PATH", default=None, help="write the mean of the accumulated frames as a Radiance *.hdr file, encoded on the device (with several combinations: of the last one)")
    ap.add_argument("--mean-png", metavar="PATH", default=None, help="write the sRGB8 encoding of the mean of the accumulated frames as a *.png file, encoded on the device (with several combinations: of the last one)")
    args = ap.parse_args(argv)
    common = {} if args.sample_count is None else {"sample_count": args.sample_count}
    with tempfile.TemporaryDirectory() as directory:
        dataset = synthetic.write_dataset(directory, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        reference = None
        if args.reference_frames > 0:
            r = _make_renderer(args, dataset, "libm", **common)
            try:
                reference = measure(r, args.reference_frames, seed=args.reference_seed, return_mean=True)["mean"]
            finally:
                r.close()
        for technique, strategy, heuristic, arithmetic, noise, ltc in itertools.product(args.technique, args.strategy, args.heuristic, args.arithmetic, args.noise, args.ltc):
            overrides = dict(common)
            for key, value in (("polygon_technique", technique), ("sampling_strategies", strategy), ("mis_heuristic", heuristic)):
                if value is not None:
                    overrides[key] = value
            line = {"config": args.config, "technique": technique, "strategy": strategy, "heuristic": heuristic, "arithmetic": arithmetic, "noise": noise, "ltc": ltc}
            r = None
            try:
                r = _make_renderer(args, dataset, arithmetic, noise, ltc, **overrides)
                extent = r.app.swapchain.extent
                line.update({"width": extent.width, "height": extent.height, "sample_count": int(r.app.render_settings.sample_count), "reference_frames": args.reference_frames})
                line.update(measure(r, args.frames, reference, seed=args.seed, mean_hdr=args.mean_hdr, mean_png=args.mean_png))
            except RuntimeError as error:
                # (a combination the pass refuses, e.g. a diffuse-only technique with an MIS strategy: its message is on stdout)
                line["error"] = str(error)
            finally:
                if r is not None:
                    r.close()
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
