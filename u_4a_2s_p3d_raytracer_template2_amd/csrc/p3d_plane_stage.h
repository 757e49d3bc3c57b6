// p3d_plane_stage.h -- how an image-space entry (p3d_denoise*, p3d_upsample, p3d_accumulate*, p3d_ambient_occlusion,
// p3d_indirect_diffuse) moves its planes between the caller's memory and the handle's buffers.  The entry
//   1. declares every plane it was given (in / out) and every buffer of the handle it needs besides (scratch);
//   2. prepares: refuse_in_capture(), then allocate() -- two steps, so that an entry can run checks of its own between
//      them and a refused call does not grow the handle;
//   3. runs: upload(), its launch on the declared planes (a Plane converts to the pointer the kernels use), finish().
// Internal: not installed with include/.
#ifndef P3D_PLANE_STAGE_H
#define P3D_PLANE_STAGE_H

#include "p3d_scene_state.h"

#pragma GCC visibility push(hidden)
namespace p3d {

// A buffer of the handle, counted in p3d_scene_stats::device_bytes at whatever size it has after the call: buffers that
// entries share (p3d_trace_rays and p3d_occluded: origin / dir) are grown here by both, and the count does not depend on
// which came first (a failed allocation leaves the buffer empty and counted as such).
inline hipError_t ensure_counted(p3d_scene* s, RawBuf& b, size_t bytes) {
    s->stats.device_bytes -= b.cap;
    const hipError_t e = b.ensure(bytes);
    s->stats.device_bytes += b.cap;
    return e;
}

class PlaneStage {
    enum Role { kIn, kOut, kScratch };
    struct Rec {
        RawBuf* buf; void* user; size_t bytes; Role role; bool host;
        bool staged() const { return host || role == kScratch; }     // the plane lives in buf
    };

public:
    static constexpr int kMaxPlanes = 24;       // p3d_accumulate_variance with everything in host memory declares 21

    // A declared plane.  Read after allocate(), it is where the kernels find the plane: the handle's buffer if the
    // caller's memory is the host's (or the plane is scratch), else the caller's pointer; nullptr if the plane is not there.
    class Plane {
        const Rec* r_;
    public:
        explicit Plane(const Rec* r = nullptr) : r_(r) {}
        template <typename T> operator T*() const { return r_ ? (T*)(r_->staged() ? r_->buf->p : r_->user) : nullptr; }
    };

    // entry: the name in the refusals; noun: what the entry "has to allocate" ("its scratch", "its staging", ...)
    PlaneStage(p3d_scene* s, const char* entry, const char* noun) : s_(s), entry_(entry), noun_(noun) {}
    PlaneStage(const PlaneStage&) = delete;             // a Plane points into its stage
    PlaneStage& operator=(const PlaneStage&) = delete;

    // An input / output plane of `bytes` at the caller's `p`, which is host memory or not; staged in `buf` if it is.
    // p NULL: the plane is not there, and only its `host` counts (the caller's memory field, whichever planes came with it).
    Plane in(RawBuf& buf, const void* p, size_t bytes, bool host) { return push({&buf, const_cast<void*>(p), bytes, kIn, host}); }
    Plane out(RawBuf& buf, void* p, size_t bytes, bool host) { return push({&buf, p, bytes, kOut, host}); }
    // A buffer of the handle's without a caller's side: scratch, spare planes, the cameras.
    Plane scratch(RawBuf& buf, size_t bytes) { return push({&buf, nullptr, bytes, kScratch, false}); }

    // While the stream is being captured: no host planes (they are copied and waited for), and nothing to allocate.
    int refuse_in_capture() const {
        if (overflow_) return fail(P3D_ERR_LIMIT, std::string(entry_) + " declares more planes than a PlaneStage holds");
        if (!stream_capturing(s_->stream)) return P3D_OK;
        if (host_)
            return fail(P3D_ERR_STATE, std::string(entry_) + " copies host planes and waits for them: not while the stream is being captured");
        for (int i = 0; i < n_; i++)
            if (planes_[i].staged() && planes_[i].bytes > planes_[i].buf->cap)
                return fail(P3D_ERR_STATE, std::string(entry_) + " has to allocate " + noun_ + ": make a call of this shape before the capture");
        return P3D_OK;
    }
    // Every declared buffer at its size, in the order of the declarations.
    int allocate() {
        for (int i = 0; i < n_; i++)
            if (planes_[i].staged()) HIP_TRY(ensure_counted(s_, *planes_[i].buf, planes_[i].bytes));
        return P3D_OK;
    }
    // The host inputs into their buffers, enqueued.
    int upload() {
        for (int i = 0; i < n_; i++)
            if (planes_[i].role == kIn && planes_[i].host)
                HIP_TRY(hipMemcpyAsync(planes_[i].buf->p, planes_[i].user, planes_[i].bytes, hipMemcpyHostToDevice, s_->stream));
        return P3D_OK;
    }
    // The host outputs back, enqueued; with any host plane, the wait: the caller's host planes have been read and
    // written when the call returns.
    int finish() {
        for (int i = 0; i < n_; i++)
            if (planes_[i].role == kOut && planes_[i].host)
                HIP_TRY(hipMemcpyAsync(planes_[i].user, planes_[i].buf->p, planes_[i].bytes, hipMemcpyDeviceToHost, s_->stream));
        if (host_) HIP_TRY(hipStreamSynchronize(s_->stream));
        return P3D_OK;
    }

private:
    Plane push(const Rec& r) {
        host_ |= r.host;
        if (r.role != kScratch && !r.user) return Plane();
        if (n_ == kMaxPlanes) { overflow_ = true; return Plane(); }
        planes_[n_] = r;
        return Plane(&planes_[n_++]);
    }
    p3d_scene* s_;
    const char *entry_, *noun_;
    Rec planes_[kMaxPlanes];
    int n_ = 0;
    bool host_ = false, overflow_ = false;
};

}  // namespace p3d
#pragma GCC visibility pop

#endif
