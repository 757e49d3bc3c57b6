"""What the AOV planes of p3d_render_aov cost: BASELINE config 2's frame (mount_low 1920x1080, depth 4, BVH, device-memory
outputs) through p3d_render, through p3d_render_aov without planes, and with depth / normal / albedo, each timed with
p3d_timer_begin / p3d_timer_end over FRAMES frames after WARMUP warm-ups, REPEATS times.  One frame at a time on one handle.
usage: python tools/aov_cost.py [FRAMES [WARMUP [REPEATS]]]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from conftest import scene_path                      # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P      # noqa: E402

FRAMES, WARMUP, REPEATS = [int(a) for a in sys.argv[1:4]] + [200, 20, 3][len(sys.argv[1:4]):]
W, H = 1920, 1080


def main():
    hs = P.HostScene(scene_path("mount_low"))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    cam = hs.camera()
    L = P.lib()
    ptr = {}
    for k, bpp in (("rgb8", 3), ("rgb32f", 12), ("hit_id", 4), ("depth", 4), ("normal", 12), ("albedo", 12)):
        p = C.c_void_p()
        assert L.p3d_device_alloc(ds.h, W * H * bpp, C.byref(p)) == 0
        ptr[k] = p.value
    colour = dict(rgb8_ptr=ptr["rgb8"], rgb32f_ptr=ptr["rgb32f"], hit_ptr=ptr["hit_id"])
    runs = {
        "p3d_render": lambda: ds.render_device(cam, max_depth=4, **colour),
        "p3d_render_aov, no planes": lambda: ds.render_aov_device(cam, max_depth=4, **colour),
        "p3d_render_aov, depth": lambda: ds.render_aov_device(cam, max_depth=4, depth_ptr=ptr["depth"], **colour),
        "p3d_render_aov, depth + normal + albedo": lambda: ds.render_aov_device(
            cam, max_depth=4, depth_ptr=ptr["depth"], normal_ptr=ptr["normal"], albedo_ptr=ptr["albedo"], **colour),
    }
    print("mount_low %dx%d depth 4 BVH, device outputs, %d frames after %d warm-ups, one frame at a time; ms per frame" % (W, H, FRAMES, WARMUP))
    for rep in range(REPEATS):
        for what, run in runs.items():
            for _ in range(WARMUP):
                run()
            ds.sync()
            ds.timer_begin()
            for _ in range(FRAMES):
                run()
            ms = ds.timer_end() / FRAMES
            print("  repeat %d  %-42s %.4f   (%s, %d tile(s) per workgroup)" % (rep, what, ms, ds.last_schedule(), ds.last_primary_tiles()))
    for p in ptr.values():
        L.p3d_device_free(ds.h, C.c_void_p(p))
    ds.close()


if __name__ == "__main__":
    main()
