// libjmid_hip.so -- the host side's memory plumbing, in one place: the rounding rule, the owning buffers of the handle, the small
// host array a call sends ahead of its kernels, and the staging of the entry points that take `mem`.  Host code only; nothing here is
// process-wide.  Included by jmid_ctx.hpp between the error helpers and the handle, whose members the owners are.
#pragma once

namespace jmid_host {

struct Block;
// (defined under the handle)
hipStream_t stream_of(jmid_ctx* h);                                              // h->stream
int reserve_block(jmid_ctx* h, Block& b, size_t need, const char* who);          // b.reserve, or ensure_arena when b is the handle's arena

// THE rounding rule: every array of every workspace starts on a multiple of 256 bytes
constexpr size_t kAlign = 256;
inline size_t align_up(size_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }
inline size_t align_up_floats(size_t floats) { return align_up(floats * sizeof(float)) / sizeof(float); }      // (a block addressed in floats)

// One array of a laid-out block: where it lies and how many elements it has, stated once by the layout function - the launches take
// the pointer, the copies the bytes.  n = 0: the call has no such array, and it reads as a null pointer
template <class T>
struct Arr {
    T* p = nullptr;
    size_t n = 0;
    size_t bytes() const { return n * sizeof(T); }
    operator T*() const { return n ? p : nullptr; }
};

// Lays arrays out one behind the other.  base null: the size only (`off` after the same takes)
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(char* b) : base(b) {}
    template <class T = float>
    T* take(size_t n) {
        T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
        off += align_up(n * sizeof(T));
        return p;
    }
    template <class T = float>
    Arr<T> arr(size_t n) {
        return Arr<T>{take<T>(n), n};
    }
};

// A grow-only block of device memory, or of pinned host memory: owns its pointer and byte count, frees in its destructor.
enum MemKind { MEM_DEVICE, MEM_PINNED };
struct Block {
    char* p = nullptr;
    size_t bytes = 0;
    MemKind kind;
    explicit Block(MemKind k = MEM_DEVICE) : kind(k) {}
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    ~Block() { (void)release(); }
    hipError_t release() {
        const hipError_t e = !p ? hipSuccess : kind == MEM_PINNED ? hipHostFree(p) : hipFree(p);
        p = nullptr;
        bytes = 0;
        return e;
    }
    // At least `need` bytes.  Growing frees the old block first, so everything enqueued on the handle's stream drains before (an owner
    // other streams work in - the arena - drains them itself: ensure_arena); the contents are lost.  `who`: the entry point that was called
    int reserve(jmid_ctx* h, size_t need, const char* who) {
        if (need <= bytes) return 0;
        if (p) {
            HIPCHK(h, hipStreamSynchronize(stream_of(h)));
            HIPCHK(h, release());
        }
        const hipError_t e = kind == MEM_PINNED ? hipHostMalloc((void**)&p, need, hipHostMallocDefault) : hipMalloc((void**)&p, need);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(h, JMID_ENOMEM, std::string(who) + ": " + (kind == MEM_PINNED ? "pinned staging" : "workspace") + " allocation of " +
                                            std::to_string(need) + " bytes failed");
        }
        bytes = need;
        return 0;
    }
    template <class T>
    T* as(size_t byte_offset = 0) const { return reinterpret_cast<T*>(p + byte_offset); }
};

// A small HOST array of 4-byte elements (the episode ids of a seeded call, the agent counts of a padded one) onto the device, on the
// handle's stream.  Through pinned staging of its own: a device-mode call may return before its copies have run, and the caller's array
// need not outlive the call.  `ev`: the last upload has left the staging.
struct HostArray {
    Block dev{MEM_DEVICE}, pin{MEM_PINNED};
    hipEvent_t ev = nullptr;
    ~HostArray() {
        if (ev) (void)hipEventDestroy(ev);
    }
    int upload(jmid_ctx* h, const void* src, int n, const char* who) {
        if (!ev) HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        const size_t need = (size_t)std::max(n, 64) * 4;
        if (need > dev.bytes || need > pin.bytes) {      // (growing drains the stream: nothing reads the old staging any more)
            if (int rc = dev.reserve(h, need, who)) return rc;
            if (int rc = pin.reserve(h, need, who)) return rc;
        } else {
            HIPCHK(h, hipEventSynchronize(ev));          // the previous upload has read the staging (an event never recorded is complete)
        }
        std::memcpy(pin.p, src, (size_t)n * 4);
        HIPCHK(h, hipMemcpyAsync(dev.p, pin.p, (size_t)n * 4, hipMemcpyHostToDevice, stream_of(h)));
        HIPCHK(h, hipEventRecord(ev, stream_of(h)));
        return 0;
    }
    template <class T>
    const T* get() const { return dev.as<const T>(); }
};

// The arrays of an entry point that takes `mem`, each stated once.  JMID_MEM_DEVICE: the kernel works on the caller's pointers and
// begin() / end() only order the handle's stream against the caller's.  JMID_MEM_HOST: every array gets a slot of `blk`; begin()
// reserves the block ONCE - before any slot address reaches a copy or a kernel -, patches the slot addresses into the argument struct
// and enqueues the uploads; end() enqueues the download of every out() and synchronises.  Copies run in the order the arrays were stated.
// `blk` the handle's arena: it grows through ensure_arena (the lanes and the captured graphs work in it).
struct Staging {
    static constexpr int kMaxSlots = 8;
    struct Slot {
        void* arg;             // where the array's device address goes (a pointer member of the launch's argument struct)
        const void* src;       // upload from (in)
        void* dst;             // download to (out); neither: scratch
        size_t bytes, off;
    };
    jmid_ctx* h;
    const bool host;
    Block& blk;
    const char* who;
    Slot slot[kMaxSlots];
    int n = 0;                 // arrays stated (more than kMaxSlots: begin() refuses)
    size_t need = 0;
    Staging(jmid_ctx* h_, int mem, Block& blk_, const char* who_) : h(h_), host(mem == JMID_MEM_HOST), blk(blk_), who(who_) {}
    int mem() const { return host ? JMID_MEM_HOST : JMID_MEM_DEVICE; }
    void add(void* arg, const void* src, void* dst, size_t bytes) {
        if (n < kMaxSlots) slot[n] = Slot{arg, src, dst, bytes, need};
        ++n;
        need += align_up(bytes);
    }
    // device_copy: the array goes into a slot in device mode too (a device-to-device copy)
    template <class T>
    void in(const T** arg, const T* src, size_t count, bool device_copy = false) {
        *arg = src;
        if (host || device_copy) add(arg, src, nullptr, count * sizeof(T));
    }
    template <class T>
    void out(T** arg, T* dst, size_t count) {
        *arg = dst;
        if (host) add(arg, nullptr, dst, count * sizeof(T));
    }
    template <class T>
    void scratch(T** arg, size_t bytes) {      // both modes
        add(arg, nullptr, nullptr, bytes);
    }
    int begin() {
        if (n > kMaxSlots) return fail(h, JMID_EINVAL, std::string(who) + ": more arrays than Staging has slots");
        if (int rc = order_in(h, mem())) return rc;
        if (int rc = reserve_block(h, blk, need, who)) return rc;
        for (int i = 0; i < n; ++i) {
            void* p = blk.p + slot[i].off;
            std::memcpy(slot[i].arg, &p, sizeof p);
            if (slot[i].src)
                HIPCHK(h, hipMemcpyAsync(p, slot[i].src, slot[i].bytes, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream_of(h)));
        }
        return 0;
    }
    int end() {
        if (host) {
            for (int i = 0; i < n; ++i)
                if (slot[i].dst) HIPCHK(h, hipMemcpyAsync(slot[i].dst, blk.p + slot[i].off, slot[i].bytes, hipMemcpyDeviceToHost, stream_of(h)));
            HIPCHK(h, hipStreamSynchronize(stream_of(h)));
        }
        return order_out(h, mem());
    }
};

}  // namespace jmid_host
