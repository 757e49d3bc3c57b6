"""What the GPU tests of the image-space entries share: one call with host inputs and device outputs, one with device
inputs and host outputs, each compared bit by bit with the all-device call on the same planes."""
import numpy as np


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32) if got.dtype == np.float32 else got != ref
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def check_host_device_split(ds, inputs, outputs, call):
    """inputs: {name: host array}; outputs: {name: a host array of the plane's shape and dtype}; call(in_ptr, in_memory,
    out_ptr, out_memory) runs the entry on ds with every input in in_memory and every output in out_memory (0 host,
    1 device), in_ptr / out_ptr: {name: address}.
    The host-in / device-out call runs on a stream with a few milliseconds of work in front of it, from pinned memory, and
    must leave that stream idle: the caller's host planes have been read when the call returns."""
    import torch
    as_torch = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a))
    ptrs = lambda d: {k: t.data_ptr() for k, t in d.items()}
    dev_in = {k: as_torch(a).cuda() for k, a in inputs.items()}
    dev_out = lambda: {k: torch.zeros_like(as_torch(a)).cuda() for k, a in outputs.items()}
    back = lambda d: {k: t.cpu().numpy().view(outputs[k].dtype) for k, t in d.items()}

    ref_t = dev_out()
    call(ptrs(dev_in), 1, ptrs(ref_t), 1)
    ds.sync()
    ref = back(ref_t)

    pinned = {k: as_torch(a).clone().pin_memory() for k, a in inputs.items()}
    got_t = dev_out()
    side = torch.cuda.Stream()
    filler = torch.zeros(1 << 26, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ds.set_stream(side.cuda_stream)
    try:
        with torch.cuda.stream(side):
            for _ in range(16):
                filler.add_(1.0)
        call(ptrs(pinned), 0, ptrs(got_t), 1)
        idle = side.query()
    finally:
        side.synchronize()
        ds.set_stream(0)
    assert idle, "host inputs, device outputs: the call returned with work pending on the scene's stream"
    for k, a in back(got_t).items():
        same_bits(a, ref[k], "host in, device out: " + k)

    host_out = {k: np.zeros_like(a) for k, a in outputs.items()}
    call(ptrs(dev_in), 1, {k: a.ctypes.data for k, a in host_out.items()}, 0)
    for k, a in host_out.items():
        same_bits(a, ref[k], "device in, host out: " + k)
    return ref
