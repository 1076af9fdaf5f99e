"""Runs entries of the experiment table, like `vulkan_renderer -e<N>` of the reference
(src/main.c:2277-2284 parses the flag, startup_application :1909-1925 applies the
experiment, advance_experiments :1948-2016 renders, times and takes the screenshot).

    python -m vulkan_renderer_amd.experiments -e 25 --data-root /path/with/data
    python -m vulkan_renderer_amd.experiments -e 25 --synthetic /tmp/vkr_data
    python -m vulkan_renderer_amd.experiments -e 25 --data-root /path/with/data --accumulate 1024
    python -m vulkan_renderer_amd.experiments -e 25 --synthetic /tmp/vkr_data --noise owen

Scene files, quicksaves, LTC fits and noise tables are looked up below the data root
with the reference's relative paths (data/attic.vks, data/quicksaves/..., data/ggx_ltc_fit,
data/noise/...).  --synthetic writes a generated stand-in data set (one synthetic scene
under every scene name, white noise instead of the Ahmed table, default light) so the
whole procedure can be exercised without the downloaded assets.  --noise TYPE replaces the experiment's noise table by
one generated on the device (blue, sobol, owen, burley_owen, blue_noise_dithered: include/vkr_noise_table.h).  The table, the path
handling, the screenshot encoders and the file writers are C code in libvkr_shading.so;
this module only sequences the calls."""
import argparse
import contextlib
import ctypes as C
import os
import sys

import numpy as np

from . import capi, renderer, synthetic


def experiment_table(lib=None):
    lib = lib or capi.load()
    table = capi.ExperimentList()
    lib.create_experiment_list(C.byref(table))
    return table


def write_synthetic_data_root(root, grid=128, box_count=32):
    """A data root with the reference's layout where every scene is the synthetic scene."""
    data = os.path.join(root, "data")
    made = synthetic.write_dataset(os.path.join(root, "synthetic"), grid=grid, box_count=box_count)
    lib = capi.load()
    paths = (C.c_char_p * 4 * 9).in_dll(lib, "g_scene_paths")
    for scene in range(9):
        scene_path = os.path.join(root, paths[scene][1].decode())
        texture_path = os.path.join(root, paths[scene][2].decode())
        os.makedirs(os.path.dirname(scene_path), exist_ok=True)
        for source, target in ((made["scene"], scene_path), (made["textures"], texture_path)):
            if not os.path.lexists(target):
                os.symlink(os.path.abspath(source), target)
    ltc = os.path.join(data, "ggx_ltc_fit")
    if not os.path.lexists(ltc):
        os.symlink(os.path.abspath(made["ltc"]), ltc)
    os.makedirs(os.path.join(data, "quicksaves"), exist_ok=True)
    os.makedirs(os.path.join(data, "experiments"), exist_ok=True)
    return {"fresnel_count": made["fresnel_count"]}


@contextlib.contextmanager
def experiment_renderer(index, data_root, synthetic_inputs=False, fresnel_count=51, hip_device=0, noise=None, ltc="synthetic"):
    """A Renderer with experiment `index` applied, its scene, tables, targets and pass created and the visibility pass
    rendered: yields (renderer, experiment) and closes both afterwards.  noise: a type that is generated on the device
    instead of the experiment's table; ltc "fitted": the LTC table is fitted on the device (fit_ltc_table, default size
    with fresnel_count slices) instead of read from data/ggx_ltc_fit"""
    lib = capi.load()
    table = experiment_table(lib)
    try:
        if not 0 <= index < table.count:
            raise ValueError("experiment index %d is not in [0, %d)" % (index, table.count))
        experiment = table.experiments[index]
        r = renderer.Renderer(hip_device=hip_device)
        try:
            if lib.apply_experiment(C.byref(r.app), C.byref(experiment), data_root.encode()):
                raise RuntimeError("apply_experiment failed")
            spec = r.app.scene_specification
            settings = r.app.render_settings
            if synthetic_inputs:
                # no Ahmed / blue noise tables without the downloaded data
                settings.noise_type = 0
                if spec.polygonal_light_count == 0:
                    r.set_lights(synthetic.config_lights(2))
                    cam = synthetic.DEFAULT_CAMERA
                    r.set_camera(cam["position"], cam["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])
            r.load_scene(C.string_at(spec.file_path).decode(), C.string_at(spec.texture_path).decode(), acceleration_structure=True)
            if ltc == "fitted":
                r.fit_ltc_table(fresnel_count=fresnel_count)
            else:
                r.load_ltc_table(os.path.join(data_root, "data", "ggx_ltc_fit"), fresnel_count)
            cwd = os.getcwd()
            os.chdir(data_root)  # noise tables are addressed relative to the working directory (noise_table.c)
            try:
                if noise is None:
                    r.load_noise_table(int(settings.noise_type))
                else:
                    settings.noise_type = renderer.NOISE[noise]
                    r.generate_noise_table(noise)
                # the quicksave may hold textured lights (reference update_application, main.c:1879);
                # their paths are relative to the working directory too
                r.create_light_textures()
            finally:
                os.chdir(cwd)
            r.create_targets()
            r.create_pass()
            r.render_visibility()
            yield r, experiment
        finally:
            r.close()
    finally:
        lib.destroy_experiment_list(C.byref(table))


def run_experiment(index, data_root, frames=32, warmup=4, synthetic_inputs=False, fresnel_count=51, hdr=False, hip_device=0, verbose=True, accumulate=0, noise=None, ltc="synthetic", jpg=False, png=True, device_hdr=False, device_png=False):
    """Renders experiment `index` and stores its screenshot.  device_png: the *.png, encoded on the device
    (take_png_screenshot): the pixels of the host writer's file in fewer bytes.  device_hdr: the *.hdr of hdr=True, encoded on the device
    (take_hdr_screenshot) with the header of the reference's writer.  jpg: a *.jpg, encoded on the device (take_jpg_screenshot), next
    to the *.png or - png=False - instead of it; like the reference (main.c:1551) not together with hdr.  Returns a dict with the
    frame time and the screenshot path, or raises with the library's message.
    accumulate = n > 0: the screenshot holds the mean of n further frames with animated noise (summed on the device,
    include/vkr_frame_statistics.h) instead of the last frame; "accumulate_seed" of the result is the noise seed
    (noise_table_t.random_seed) of the first of them."""
    lib = capi.load()
    with experiment_renderer(index, data_root, synthetic_inputs, fresnel_count, hip_device, noise, ltc) as (r, experiment):
        settings = r.app.render_settings
        wants_rays = bool(settings.trace_shadow_rays)
        for _ in range(warmup):
            r.render()
        r.sync()
        for _ in range(frames):
            r.render()
        r.sync()
        times = sorted(r.dispatch_ms(frames))
        frame_ms = times[len(times) // 2]
        accumulate_seed = None
        if accumulate > 0:
            accumulate_seed = int(r.app.noise_table.random_seed)
            animate_before = settings.animate_noise
            settings.animate_noise = 1
            statistics = r.create_statistics()
            for _ in range(accumulate):
                r.render()
                statistics.accumulate()
            # the converged image takes the place of the last frame: the screenshot path below is the usual one
            statistics.resolve(r.app.render_targets.radiance, None)
            statistics.close()
            settings.animate_noise = animate_before
        hdr = hdr or device_hdr
        if jpg and hdr:
            raise ValueError("*.jpg and *.hdr screenshots cannot be mixed")
        screenshot = C.string_at(experiment.screenshot_path).decode()
        if hdr:
            screenshot = screenshot[:-3] + "hdr"
        pointer = lib.format_screenshot_path(os.path.join(data_root, screenshot).encode(), frame_ms)
        path = C.string_at(pointer).decode()
        C.CDLL(None).free(C.c_void_p(pointer))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if device_hdr:
            if lib.take_hdr_screenshot(C.byref(r.app), path.encode()):
                raise RuntimeError("take_hdr_screenshot failed for %s" % path)
        elif device_png and not hdr and (png or not jpg):
            if lib.take_png_screenshot(C.byref(r.app), path.encode()):
                raise RuntimeError("take_png_screenshot failed for %s" % path)
        elif (hdr or png or not jpg) and lib.take_screenshot(C.byref(r.app), None if hdr else path.encode(), path.encode() if hdr else None):
            raise RuntimeError("take_screenshot failed for %s" % path)
        path_jpg = path[:-3] + "jpg" if jpg else None
        if jpg and lib.take_jpg_screenshot(C.byref(r.app), path_jpg.encode()):
            raise RuntimeError("take_jpg_screenshot failed for %s" % path_jpg)
        result = {"index": index, "frame_ms": frame_ms, "screenshot": path, "width": r.app.swapchain.extent.width,
                  "height": r.app.swapchain.extent.height, "rays": bool(wants_rays and r.app.shading_pass.use_ray_tracing),
                  "Msamples_per_s": r.app.swapchain.extent.width * r.app.swapchain.extent.height * settings.sample_count / (frame_ms * 1e-3) / 1e6}
        if jpg:
            result["screenshot_jpg"] = path_jpg
        if noise is not None:
            result["noise"] = noise
        if ltc != "synthetic":
            result["ltc"] = ltc
        if accumulate > 0:
            result.update({"accumulated_frames": int(accumulate), "accumulate_seed": accumulate_seed})
        if verbose:
            print(result)
        return result


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-e", "--experiment", type=int, default=None, help="index into the experiment table; omit to list the table")
    ap.add_argument("--data-root", default=".", help="directory that contains data/ (the reference's working directory)")
    ap.add_argument("--synthetic", metavar="DIR", default=None, help="write a generated stand-in data root to DIR and use it")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--hdr", action="store_true", help="store *.hdr instead of *.png (take_hdr_screenshots of the reference)")
    ap.add_argument("--device-hdr", action="store_true", help="store the *.hdr of --hdr, encoded on the device, with the header of the reference's writer")
    ap.add_argument("--device-png", action="store_true", help="store the *.png encoded on the device: the same pixels and filtered rows, dynamic Huffman codes")
    ap.add_argument("--jpg", action="store_true", help="store a *.jpg, encoded on the device at quality 70, next to the *.png (not with --hdr)")
    ap.add_argument("--no-png", action="store_true", help="with --jpg: store the *.jpg instead of the *.png")
    ap.add_argument("--accumulate", type=int, default=0, metavar="N", help="store the mean of N frames with animated noise instead of the last frame")
    ap.add_argument("--noise", default=None, choices=["blue", "sobol", "owen", "burley_owen", "blue_noise_dithered"], help="generate this noise table on the device instead of loading the experiment's")
    ap.add_argument("--ltc", default="synthetic", choices=["synthetic", "fitted"], help="fitted: fit the LTC table on the device instead of reading data/ggx_ltc_fit (synthetic: the files of the data root, which --synthetic fills with placeholder fits)")
    args = ap.parse_args(argv)
    if args.jpg and (args.hdr or args.device_hdr):
        ap.error("--jpg and --hdr cannot be mixed")
    lib = capi.load()
    if args.experiment is None:
        table = experiment_table(lib)
        for i in range(table.count):
            print("%03d: %s" % (i, table.experiments[i].screenshot_path.decode()))
        lib.destroy_experiment_list(C.byref(table))
        return 0
    fresnel_count = 51
    root = args.data_root
    if args.synthetic:
        root = args.synthetic
        fresnel_count = write_synthetic_data_root(root)["fresnel_count"]
    run_experiment(args.experiment, root, frames=args.frames, synthetic_inputs=bool(args.synthetic), fresnel_count=fresnel_count, hdr=args.hdr, accumulate=args.accumulate, noise=args.noise, ltc=args.ltc, jpg=args.jpg, png=not (args.jpg and args.no_png), device_hdr=args.device_hdr, device_png=args.device_png)
    return 0


if __name__ == "__main__":
    sys.exit(main())
