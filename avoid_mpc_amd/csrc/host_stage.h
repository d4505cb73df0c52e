// Staging of the host-memory (*_host) entry points of the C ABI: one block of device memory per handle, laid out afresh by every
// call.  Included by amk_common.h (AMK_HIP above it), ahead of the handles that hold a HostStage.
#pragma once
#include <cstring>
#include <initializer_list>
#include <vector>

namespace amk {

// One copy between host and device memory.  As a slot of a staged call (HostStage): `bytes` of device storage (0: none, the launch gets a null pointer), filled from the host
// memory `src` before the launch (null: not filled) and copied to the host memory `dst` after the wait (null: not wanted).
// As a read-back from a handle's own device array (read_back): `src` on the device, `dst` on the host (null: not wanted).
struct HostCopy { void *dst; const void *src; size_t bytes; };
inline HostCopy to_device(const void *h, size_t bytes) { return {nullptr, h, bytes}; }
inline HostCopy to_host(void *h, size_t bytes) { return {h, nullptr, bytes}; }
inline HostCopy both_ways(void *h, size_t bytes) { return {h, h, bytes}; }
inline HostCopy scratch(size_t bytes) { return {nullptr, nullptr, bytes}; }
// for a launch that takes "null: not given / not wanted" itself: no device storage without a host side
inline HostCopy if_given(HostCopy c) { return {c.dst, c.src, c.dst || c.src ? c.bytes : 0}; }

// Slots lie in call order at multiples of 256 bytes, as separate hipMallocs would; `end` runs along (amk__stage_layout is this loop)
inline size_t stage_next(size_t &end, size_t bytes) {
    const size_t offset = (end + 255) / 256 * 256;
    if (bytes) end = offset + bytes;   // (an empty slot takes no room, not even the padding in front of it)
    return offset;
}

// The read-backs: a device-wide wait, then the wanted copies out of the handle's arrays
inline int read_back(std::initializer_list<HostCopy> out) {
    AMK_HIP(hipDeviceSynchronize());
    for (const HostCopy &c : out)
        if (c.dst && c.bytes) AMK_HIP(hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost));
    return AMK_OK;
}
// n points of three coordinate planes on the device -> packed xyz on the host (no wait of its own)
inline int planes_to_xyz(const float *d_x, const float *d_y, const float *d_z, int n, float *h_xyz) {
    if (n <= 0) return AMK_OK;
    std::vector<float> plane((size_t)n);
    const float *src[3] = {d_x, d_y, d_z};
    for (int c = 0; c < 3; ++c) {
        AMK_HIP(hipMemcpy(plane.data(), src[c], sizeof(float) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) h_xyz[(size_t)i * 3 + c] = plane[i];
    }
    return AMK_OK;
}

// Copy the inputs in, launch with the slots' device pointers, wait, copy the wanted outputs back.  The blocks grow on demand and
// never shrink; every call ends in its wait, so the next call of the handle may lay the block out anew.
class HostStage {
public:
    static constexpr int kMaxSlots = 12;   // amk_sim_path_cast_host: the world's four arrays, the path and seven outputs
    // a slot's device pointer, taken as whatever pointer the launch's parameter is
    struct Dev { unsigned char *p = nullptr; template <class T> operator T *() const { return reinterpret_cast<T *>(p); } };
    HostStage() = default;
    HostStage(const HostStage &) = delete;
    ~HostStage() {
        if (dev_) (void)hipFree(dev_);
        if (pin_) (void)hipHostFree(pin_);
        if (stream_) (void)hipStreamDestroy(stream_);
    }

    // blocking copies; launch(d) enqueues on the null stream, d[i] = slot i; wait() is the entry's own (device-wide or null stream)
    template <class Launch>
    int call(std::initializer_list<HostCopy> slots, Launch &&launch, hipError_t (*wait)()) {
        const HostCopy *c = slots.begin();
        const int n = (int)slots.size();
        if (const int st = place(c, n, false); st != AMK_OK) return st;
        for (int i = 0; i < n; ++i)
            if (c[i].src && c[i].bytes) AMK_HIP(hipMemcpy(dev_ + offset_[i], c[i].src, c[i].bytes, hipMemcpyHostToDevice));
        if (const int st = launch(d_); st != AMK_OK) return st;
        AMK_HIP(wait());
        for (int i = 0; i < n; ++i)
            if (c[i].dst && c[i].bytes) AMK_HIP(hipMemcpy(c[i].dst, dev_ + offset_[i], c[i].bytes, hipMemcpyDeviceToHost));
        return AMK_OK;
    }

    // The same through a pinned host block of the same layout and a private non-blocking stream: one memcpy per input, ONE copy
    // in (the block up to its last input), launch(d, stream), ONE copy out (every slot behind the last input, wanted or not) and
    // a wait on this stream only -- no other stream of the process is stalled.  The inputs are the leading slots.
    template <class Launch>
    int call_pinned(std::initializer_list<HostCopy> slots, Launch &&launch) {
        const HostCopy *c = slots.begin();
        const int n = (int)slots.size();
        if (const int st = place(c, n, true); st != AMK_OK) return st;
        size_t in_end = 0, out_begin = n > 0 ? offset_[0] : total_;
        for (int i = 0; i < n; ++i) {
            if (!c[i].src || !c[i].bytes) continue;
            std::memcpy(pin_ + offset_[i], c[i].src, c[i].bytes);
            in_end = offset_[i] + c[i].bytes;
            out_begin = i + 1 < n ? offset_[i + 1] : total_;
        }
        if (in_end) AMK_HIP(hipMemcpyAsync(dev_, pin_, in_end, hipMemcpyHostToDevice, stream_));
        if (const int st = launch(d_, stream_); st != AMK_OK) return st;
        if (out_begin < total_) AMK_HIP(hipMemcpyAsync(pin_ + out_begin, dev_ + out_begin, total_ - out_begin, hipMemcpyDeviceToHost, stream_));
        AMK_HIP(hipStreamSynchronize(stream_));
        for (int i = 0; i < n; ++i)
            if (c[i].dst && c[i].bytes) std::memcpy(c[i].dst, pin_ + offset_[i], c[i].bytes);
        return AMK_OK;
    }

private:
    // the recorded size changes only behind a successful allocation: a failed growth leaves the block empty
    static int grow(unsigned char *&p, size_t &bytes, size_t want, bool pinned) {
        if (bytes >= want) return AMK_OK;
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
        void *fresh = nullptr;
        AMK_HIP(pinned ? hipHostMalloc(&fresh, want, hipHostMallocDefault) : hipMalloc(&fresh, want));
        p = static_cast<unsigned char *>(fresh);
        bytes = want;
        return AMK_OK;
    }
    // this call's layout (offset_, total_), the blocks grown to hold it, d_[i] = slot i's device pointer
    int place(const HostCopy *c, int n, bool pinned) {
        if (n > kMaxSlots) return AMK_ERR_UNSUPPORTED;
        total_ = 0;
        for (int i = 0; i < n; ++i) offset_[i] = stage_next(total_, c[i].bytes);
        if (const int st = grow(dev_, dev_bytes_, total_, false); st != AMK_OK) return st;
        if (pinned && !stream_) AMK_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        if (const int st = pinned ? grow(pin_, pin_bytes_, total_, true) : AMK_OK; st != AMK_OK) return st;
        for (int i = 0; i < n; ++i) d_[i].p = c[i].bytes ? dev_ + offset_[i] : nullptr;
        return AMK_OK;
    }

    unsigned char *dev_ = nullptr, *pin_ = nullptr;
    size_t dev_bytes_ = 0, pin_bytes_ = 0, offset_[kMaxSlots], total_ = 0;
    Dev d_[kMaxSlots];
    hipStream_t stream_ = nullptr;
};

}  // namespace amk
