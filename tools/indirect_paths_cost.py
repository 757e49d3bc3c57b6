#!/usr/bin/env python3
"""What p3d_indirect_paths costs (profiles/indirect_paths_cost.txt): mount_low (served from LDS) and dragon (read from HBM) at
1920x1080, accel BVH, 4 and 16 paths per pixel, 1, 2 and 4 bounces, everything in device memory, one process.  Timed with
p3d_timer_begin / p3d_timer_end over CALLS calls after WARMUP warm-ups; the cases alternate REPEATS times and each figure is
the median.
  (a) the fused entry, writing the indirect plane.
  (b) the unfused composition: B rounds of p3d_trace_rays(max_depth = 1) on COMPACTED rays in device memory -- vertex 0's
      rays made once by the host restatement (api.host_ao_segments at radius 1), neither making nor uploading them is
      timed -- with the steps between two rays (the definition's step 3 and 4: hit point, albedo look-up, throughput,
      face-forward, the keyed rejection draw, compaction of the paths that ended) as torch elementwise operations on the
      same stream, and the definition's tree over the samples at the end.  The rejection draw stops at the first try after
      which no path is still drawing, as the kernel's ballot does; that test, and every compaction, reads a count back.
  (c) p3d_indirect_diffuse at the same S: the floor, B = 1.
Before anything is timed the fused plane is compared, every bit, with (b)'s; (b) also tells the share of paths alive at each
bounce.
usage: python tools/indirect_paths_cost.py [CALLS [WARMUP [REPEATS [WIDTH HEIGHT]]]]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

import ao_reference as AO  # noqa: E402
from extra_scenes import scene_path  # noqa: E402
import torch  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P  # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api  # noqa: E402

ARGS = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
CALLS, WARMUP, REPEATS = ARGS[:3] + [5, 1, 3][len(ARGS[:3]):]
W, H = ARGS[3:5] if len(ARGS) >= 5 else (1920, 1080)
BIAS, SEED = api.INDIRECT_BIAS, 1
M32 = 0xFFFFFFFF
TINY = 2.0 ** -20


def timed(ds, run):
    for _ in range(WARMUP):
        run()
    ds.sync()
    ds.timer_begin()
    for _ in range(CALLS):
        run()
    return ds.timer_end() / CALLS


# ---- the definition's integer and float steps on device tensors: uint32 arithmetic in int64 under a mask, float32 basic
# operations one launch each (nothing is contracted)
def rng_mix(a, b):
    h = (((a ^ 0x9E3779B9) * 0x85EBCA6B) + b) & M32
    h = h ^ (h >> 16); h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15); h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def rng_u01(key, k):
    return (rng_mix(key, k) >> 8).to(torch.float32) * (2.0 ** -24)


def normalized(a):
    s = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    return a * (1.0 / torch.sqrt(s))[:, None]


def cosine_direction(Ns, key):
    v = Ns.clone()
    accepted = torch.zeros(len(Ns), dtype=torch.bool, device=Ns.device)
    for j in range(32):
        c = torch.stack([2.0 * rng_u01(key, 3 * j + i) - 1.0 for i in range(3)], dim=1)
        q = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        take = ~accepted & (q <= 1.0) & (q >= TINY)
        v = torch.where(take[:, None], normalized(c), v)
        accepted |= take
        if bool(accepted.all()):
            break
    w = Ns + v
    ww = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    w = torch.where((ww >= TINY)[:, None], w, Ns)
    return normalized(w) * 1.0


class Unfused:
    """(b) for one scene and sample count: the buffers are allocated once, a call runs `bounces` rounds."""

    def __init__(self, ds, o, d, pk0, sample, prim_material, materials12, samples):
        self.ds, self.n, self.S = ds, len(o), samples
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.o0, self.d0 = dev(o), dev(d)
        self.pk0, self.sample = dev(pk0.astype(np.int64)), dev(sample.astype(np.int64))
        self.albedo = dev(materials12[:, 0:3])[dev(prim_material.astype(np.int64))]          # per primitive
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device="cuda:0")
        self.rgb, self.nrm, self.t = f32(self.n, 3), f32(self.n, 3), f32(self.n)
        self.hit = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        self.alive_share = []

    def __call__(self, bounces):
        n, ds = self.n, self.ds
        o, d = self.o0, self.d0
        live = None                                           # indices of the paths still alive; None: all of them
        total, T = None, None
        self.alive_share = []
        for b in range(bounces):
            m = len(o)
            self.alive_share.append(m / n)
            if m == 0:
                break
            o, d = o.contiguous(), d.contiguous()
            ds.trace_rays_device(m, o.data_ptr(), d.data_ptr(), rgb32f_ptr=self.rgb.data_ptr(), hit_ptr=self.hit.data_ptr(), t_ptr=self.t.data_ptr(),
                                 normal_ptr=self.nrm.data_ptr(), max_depth=1, accel=P.ACCEL_BVH)
            r = self.rgb[:m]
            if b == 0:
                total = r.clone()
            else:
                total[live] = total[live] + T * r
            if b + 1 == bounces:
                break
            hit = self.hit[:m].to(torch.int64)
            keep = torch.nonzero(hit >= 0)[:, 0]                                             # compaction: reads a count back
            hit, o, d, t, N = hit[keep], o[keep], d[keep], self.t[:m][keep], self.nrm[:m][keep]
            a = self.albedo[hit]
            T = a if b == 0 else T[keep] * a
            live = keep if live is None else live[keep]
            Pt = o + d * t[:, None]
            away = ((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2]) > 0
            Ns = torch.where(away[:, None], -N, N)
            o = Pt + Ns * BIAS
            key = rng_mix(rng_mix(self.pk0[live], 0x80000000 + b + 1), self.sample[live])
            d = cosine_direction(Ns, key)
        t = total.view(-1, self.S, 3)
        while t.shape[1] > 1:
            t = t[:, 0::2] + t[:, 1::2]
        return t[:, 0] * (1.0 / self.S)


def measure(name, samples, bounce_counts):
    hs = P.HostScene(scene_path(name))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    cam = hs.camera()
    arrays = hs.arrays()
    f = ds.render_aov(cam, max_depth=1, accel=P.ACCEL_BVH)
    depth, normal = f["depth"][0], f["normal"][0]
    dev = {k: torch.from_numpy(np.ascontiguousarray(f[k][0])).cuda() for k in ("depth", "normal")}
    ind = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    o, d, valid = api.host_ao_segments(cam, depth, normal, samples=samples, radius=1.0, bias=BIAS, seed=SEED)
    m = valid.astype(bool)
    o, d = np.ascontiguousarray(o[m].reshape(-1, 3)), np.ascontiguousarray(d[m].reshape(-1, 3))
    pix = (np.arange(H, dtype=np.uint32)[:, None] * np.uint32(W) + np.arange(W, dtype=np.uint32)[None, :]).astype(np.uint32)
    pk0 = np.repeat(AO.rng_mix(np.uint32(SEED), pix)[m], samples)
    sample = np.tile(np.arange(samples, dtype=np.uint32), int(m.sum()))
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)                       # one stream for the library's launches and the tool's
    with torch.cuda.stream(stream):
        unfused = Unfused(ds, o, d, pk0, sample, arrays[2], arrays[3], samples)
        where = torch.from_numpy(np.nonzero(m.ravel())[0]).cuda()
        floor = lambda: ds.indirect_diffuse_device(cam, dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_indirect_ptr=ind.data_ptr(),
                                                   samples=samples, bias=BIAS, seed=SEED, accel=P.ACCEL_BVH)
        for B in bounce_counts:
            fused = lambda B=B: ds.indirect_paths_device(cam, dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_indirect_ptr=ind.data_ptr(),
                                                         samples=samples, bounces=B, bias=BIAS, seed=SEED, accel=P.ACCEL_BVH)
            ref = torch.zeros(H * W, 3, dtype=torch.float32, device="cuda:0")
            ref[where] = unfused(B)
            share = list(unfused.alive_share)
            fused()
            ds.sync()
            equal = bool(torch.equal(ind.view(torch.int32), ref.view(-1).view(torch.int32)))
            print("%s S=%d B=%d: %.1f %% of the pixels have a path, %d paths; share of them alive at each bounce: %s; fused == unfused composition "
                  "in every bit: %s" % (name, samples, B, 100 * m.mean(), len(o), " ".join("%.3f" % s for s in share), equal), flush=True)
            assert equal, "%d values differ" % int((ind.view(torch.int32) != ref.view(-1).view(torch.int32)).sum())
            cases = [("(a) fused", fused), ("(b) unfused", lambda B=B: unfused(B)), ("(c) indirect_diffuse", floor)]
            ms = {k: [] for k, _ in cases}
            for rep in range(REPEATS):
                for k, run in cases:
                    ms[k].append(timed(ds, run))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            for k, _ in cases:
                print("  %-10s S=%-2d B=%d %-20s %9.4f ms  (%s)" % (name, samples, B, k, med[k], " ".join("%.4f" % v for v in ms[k])))
            print("  %-10s S=%-2d B=%d (a) / (b) = %.3f   (a) / (B x (c)) = %.3f   (a) / (c) = %.3f"
                  % (name, samples, B, med["(a) fused"] / med["(b) unfused"], med["(a) fused"] / (B * med["(c) indirect_diffuse"]),
                     med["(a) fused"] / med["(c) indirect_diffuse"]), flush=True)
    ds.set_stream(0)
    ds.close()


def main():
    print("library: %s" % os.path.relpath(api.LIB_PATH, REPO))
    print("%dx%d, accel BVH, bias %g, device memory, %d calls after %d warm-ups, %d alternated repetitions, medians"
          % (W, H, BIAS, CALLS, WARMUP, REPEATS))
    for name in ("mount_low", "dragon"):
        for samples in (4, 16):
            measure(name, samples, (1, 2, 4))


if __name__ == "__main__":
    main()
