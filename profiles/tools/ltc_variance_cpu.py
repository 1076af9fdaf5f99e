"""What the fitted LTC table does to the variance on the CPU oracle: config 3 and a glossy variant (roughness_factor 0.3) of
the test-suite's scene at 256x144, 64 frames of animated noise, the synthetic table against a 16 x 16 x 8 table fitted by
the numpy restatement (vulkan_renderer_amd/ltc_fit.py; the device gives the same bits).  One JSON line per combination.

    python profiles/tools/ltc_variance_cpu.py out.jsonl"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from helpers import oracle_render
from vulkan_renderer_amd import ltc_fit, renderer, synthetic

if __name__ == "__main__":
    out = open(sys.argv[1], "w")
    with tempfile.TemporaryDirectory() as d:
        dataset = synthetic.write_dataset(d, grid=64, box_count=24, seed=1234, ltc_resolution=16, fresnel_count=8)
        t = time.time()
        fits = ltc_fit.fit_table(16, 8, 32, 200, processes=16)
        print("numpy fit of 16x16x8: %.1f s" % (time.time() - t), flush=True)
        fitted = os.path.join(d, "fitted")
        ltc_fit.write_fits(fitted, fits)
        for roughness_factor in (1.0, 0.3):
            for strategy, heuristic in (("diffuse_specular_separately", "balance"), ("diffuse_specular_mis", "balance"), ("diffuse_specular_mis", "weighted"), ("diffuse_specular_mis", "optimal_clamped")):
                for ltc in ("synthetic", "fitted"):
                    hs = renderer.HostScene()
                    renderer.setup_config(hs, 3, dataset, width=256, height=144, sampling_strategies=strategy, mis_heuristic=heuristic, animate_noise=True)
                    if ltc == "fitted":
                        hs.lib.destroy_ltc_table(C.byref(hs.app.ltc_table), None)
                        hs.load_ltc_table(fitted, 8)
                    hs.app.render_settings.roughness_factor = roughness_factor
                    hs.app.noise_table.random_seed = 1000
                    total, squares, bvh, visibility = None, None, None, None
                    for k in range(64):
                        image, inputs, bvh = oracle_render(hs, visibility=visibility, math_mode=0, bvh=bvh)
                        visibility = inputs["visibility"]
                        rgb = image[..., :3].astype(np.float64)
                        total = rgb if total is None else total + rgb
                        squares = rgb * rgb if squares is None else squares + rgb * rgb
                    variance = (squares - total * total / 64) / 63
                    line = {"where": "cpu oracle", "config": 3, "width": 256, "height": 144, "frames": 64, "roughness_factor": roughness_factor, "strategy": strategy, "heuristic": heuristic, "ltc": ltc, "mean_variance": float(variance.mean())}
                    print(json.dumps(line), flush=True)
                    out.write(json.dumps(line) + "\n"); out.flush()
                    hs.close()
