"""What p3d_scene_build_grid costs against the path a moving scene in GRID mode had before it: the lazy host build.  Per scene
(mount_low, dragon, the synthetic scaling scene of PRIMS primitives), on one handle, REPEATS times, alternated:
  host    p3d_scene_update of every primitive from HOST memory (drops the grid, refreshes the host's boxes), p3d_sync, then
          the timed call: a GRID-mode p3d_occluded of one segment -- build_grid() on one host thread, two synchronous uploads
          and one tiny launch
  device  p3d_scene_update of every primitive from DEVICE memory (drops the grid), p3d_sync, then the timed call:
          p3d_scene_build_grid
Host clock around the synchronous calls; one untimed round of each first (allocations, code objects, the sort's tuning).
The geometry does not change between rounds, so both paths build the same grid: its dims and totals are printed once.
usage: python tools/grid_build_cost.py [PRIMS [REPEATS]]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from extra_scenes import scene_path                  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P      # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api, synthetic as SY      # noqa: E402

PRIMS, REPEATS = [int(a) for a in sys.argv[1:3]] + [1000000, 3][len(sys.argv[1:3]):]


def handle(name):
    """-> (DeviceScene, prim_data [n, 12])"""
    if name == "synthetic":
        arrays = SY.arrays(PRIMS)
        desc, keep = api.make_desc(*arrays)
        return P.DeviceScene(desc, keepalive=keep), np.ascontiguousarray(arrays[1], np.float32).reshape(-1, 12)
    hs = P.HostScene(scene_path(name))
    return P.DeviceScene.from_host(hs), np.ascontiguousarray(hs.arrays()[1], np.float32)


def measure(name):
    ds, data = handle(name)
    n = len(data)
    L = P.lib()
    d_data = C.c_void_p()
    assert L.p3d_device_alloc(ds.h, data.nbytes, C.byref(d_data)) == 0 and L.p3d_upload(ds.h, d_data, data.ctypes.data, data.nbytes) == 0
    o, d = np.zeros((1, 3), np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)

    def host():
        ds.update(data)
        ds.sync()
        t0 = time.perf_counter()
        ds.occluded(o, d, accel=P.ACCEL_GRID)
        return (time.perf_counter() - t0) * 1e3

    def device():
        ds.update_device(n, d_data.value)
        ds.sync()
        t0 = time.perf_counter()
        info = ds.build_grid()
        ms = (time.perf_counter() - t0) * 1e3
        assert info["built"] == 1
        return ms, info

    host()
    _, info = device()
    name_n = "%s (%d primitives)" % (name, n)
    out = ["  %-34s grid %d x %d x %d = %d cells, %d references" % ((name_n,) + tuple(int(v) for v in info["n"]) + (info["n_cells"], info["n_items"]))]
    ms = {"host": [], "device": []}
    for rep in range(REPEATS):
        ms["host"].append(host())
        ms["device"].append(device()[0])
        out.append("  repeat %d  %-12s lazy host build (p3d_occluded, 1 segment) %10.3f ms    p3d_scene_build_grid %9.3f ms" % (
            rep, name, ms["host"][-1], ms["device"][-1]))
    out.append("            %-12s host / device, medians: %.1f x" % (name, np.median(ms["host"]) / np.median(ms["device"])))
    L.p3d_device_free(ds.h, d_data)
    ds.close()
    return out


def main():
    print("GRID mode's grid after every primitive was updated: the lazy host build against p3d_scene_build_grid, %d alternated repeats" % REPEATS)
    for name in ("mount_low", "dragon", "synthetic"):
        print("\n".join(measure(name)), flush=True)


if __name__ == "__main__":
    main()
