// The protocol of the resident waves: ONE wave stays on a CU and answers requests that the host posts in pinned,
// device-mapped host memory, so that one point is evaluated without a launch.  Three features use it - the model's per-point
// lnpost callback (IsoMailbox, iso_fast_mailbox.hip), an observation tree's (IsoTreeBox, iso_fast_tree.hip) and the scalar
// accessors' service wave (IsoSvcBox, kernels/k_service.h).  Each box has its own request and result words and these
// shared control lines:
//
//   req[0]   sequence word, written LAST behind the request's other words; its high 32 bits are mailbox_checksum of them,
//            so that a request whose words did not arrive together is polled again instead of evaluated
//   done[0]  the sequence word of the last finished request: the device writes its results, a system fence, then done[0]
//   ctl[0]   state: ISO_WAVE_NONE / _RUNNING (the host, before a launch) / _EXITED (the device, when it leaves)
//   ctl[1]   quit: the host asks the wave to leave
//
// The wave leaves after ISOCHRONES_AMD_MAILBOX_IDLE_US without a request (default 1000 us, at least 10: the longest a
// device-wide synchronise elsewhere in the process is held up by it), after ISO_WAVE_LIFE_S whatever happens, or when told.
// The host relaunches it on the next request.  ISOCHRONES_AMD_MAILBOX=0 keeps every call on the launch path.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace iso {

constexpr unsigned long long ISO_WAVE_NONE = 0, ISO_WAVE_RUNNING = 1, ISO_WAVE_EXITED = 2;   // ctl[0]
constexpr double ISO_WALL_CLOCK_HZ = 1.0e8;      // wall_clock64(): the constant 100 MHz counter
constexpr double ISO_WAVE_LIFE_S = 30.0;         // a wave leaves after this long whatever happens

// 32-bit checksum of a request's n words (host and device compute the same number); word(q) gives word q
template <class Word>
__host__ __device__ inline uint32_t mailbox_checksum(int n, Word word)
{
    uint32_t c = 0x9E3779B9u;
    for (int q = 0; q < n; ++q) {
        const unsigned long long x = word(q);
        c = (c ^ (uint32_t)x) * 0x85EBCA6Bu;
        c = (c ^ (uint32_t)(x >> 32)) * 0xC2B2AE35u + (uint32_t)q;
    }
    return c;
}
__host__ __device__ inline uint32_t mailbox_checksum(const unsigned long long* w, int n)
{
    return mailbox_checksum(n, [w](int q) { return w[q]; });
}

// ---- device side -------------------------------------------------------------------------------------------------------------
// the box's words are read and written with system-scope atomics (the host reads and writes them while the wave runs)
__device__ __forceinline__ unsigned long long sys_load(const unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_store(unsigned long long* p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The polling loop's state and its three steps; every test is wave-uniform (all lanes read the same words):
//   WaveLoop<Box> W(mb, idle_ticks, life_ticks);
//   for (;;) {
//       seq = <req[0], as read by the poll>;
//       if (seq == W.last) { if (W.leave()) break; continue; }
//       <evaluate, write the results>;
//       W.answered(seq, lane);
//   }
//   W.exit(lane);
template <class Box>
struct WaveLoop {
    Box* mb;
    unsigned long long idle_ticks, life_ticks;
    unsigned long long last;           // what the previous resident wave (or nobody) finished last
    unsigned long long t_start, t_idle;

    __device__ __forceinline__ WaveLoop(Box* box, unsigned long long idle, unsigned long long life)
        : mb(box), idle_ticks(idle), life_ticks(life), last(sys_load(&box->done[0])), t_start(wall_clock64()), t_idle(t_start)
    {
    }
    // nothing new: idle too long, alive too long, or told to quit
    __device__ __forceinline__ bool leave() const
    {
        const unsigned long long now = wall_clock64();
        return (now - t_idle > idle_ticks) | (now - t_start > life_ticks) | (sys_load(&mb->ctl[1]) != 0);
    }
    // the request's results are written: its sequence word behind them
    __device__ __forceinline__ void answered(unsigned long long seq, int lane)
    {
        __threadfence_system();
        if (lane == 0) sys_store(&mb->done[0], seq);
        last = seq;
        t_idle = wall_clock64();
    }
    __device__ __forceinline__ void exit(int lane)
    {
        __threadfence_system();
        if (lane == 0) sys_store(&mb->ctl[0], ISO_WAVE_EXITED);
    }
};

// ---- host side ---------------------------------------------------------------------------------------------------------------
// read on every call: tests switch it between calls
inline bool resident_waves_enabled()
{
    const char* e = std::getenv("ISOCHRONES_AMD_MAILBOX");
    return !(e && e[0] == '0');
}

// One owner's wave and its box (a model, a tree model, a context's service).  The owner serialises its calls.
template <class Box>
struct ResidentWave {
    Box* box = nullptr;              // pinned, device-mapped
    Box* d_box = nullptr;            // its device address
    hipStream_t stream = nullptr;    // non-blocking: the resident wave must not order itself against the null stream
    unsigned long long count = 0;    // requests posted
    int state = 0;                   // 0 untried, 1 usable, -1 not available for this owner
    bool launched = false;           // a wave has been started in this box

    static unsigned long long load(const volatile unsigned long long* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }

    // lazily, on the first call: the box and its stream if usable() - the owner's own conditions, asked once; false = no wave
    // for this owner (the caller takes the launch path)
    template <class Usable>
    bool ready(Usable&& usable)
    {
        if (state != 0) return state > 0;
        state = -1;
        if (!usable()) return false;
        if (hipHostMalloc(reinterpret_cast<void**>(&box), sizeof(Box), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            box = nullptr;
            return false;
        }
        std::memset(box, 0, sizeof(Box));
        box->ctl[0] = ISO_WAVE_EXITED;               // no wave yet
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&d_box), box, 0) != hipSuccess ||
            hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostFree(box);
            box = nullptr;
            return false;
        }
        state = 1;
        return true;
    }

    // launch(d_box, idle_ticks, life_ticks, stream) starts the owner's kernel; false = no kernel for the shape
    template <class Launch>
    bool start(Launch&& launch)
    {
        double idle_us = 1000.0;
        if (const char* e = std::getenv("ISOCHRONES_AMD_MAILBOX_IDLE_US")) idle_us = std::max(10.0, std::atof(e));
        const unsigned long long idle = (unsigned long long)(idle_us * 1e-6 * ISO_WALL_CLOCK_HZ);
        const unsigned long long life = (unsigned long long)(ISO_WAVE_LIFE_S * ISO_WALL_CLOCK_HZ);
        __atomic_store_n(&box->ctl[1], 0ull, __ATOMIC_RELAXED);
        __atomic_store_n(&box->ctl[0], ISO_WAVE_RUNNING, __ATOMIC_RELEASE);       // the wave writes EXITED when it leaves
        if (!launch(d_box, idle, life, stream) || hipGetLastError() != hipSuccess) {
            __atomic_store_n(&box->ctl[0], ISO_WAVE_EXITED, __ATOMIC_RELEASE);
            return false;
        }
        launched = true;
        return true;
    }

    // The request's other words are written: post its sequence word and wait for the answer.  true = answered; false = not
    // served (the caller launches instead).  A wave whose first launch fails is not available for this owner from then on.
    template <class Launch>
    bool call(unsigned long long seq, Launch&& launch)
    {
        __atomic_store_n(&box->req[0], seq, __ATOMIC_RELEASE);        // the sequence word last
        if (load(&box->ctl[0]) != ISO_WAVE_RUNNING && !start(launch)) {
            if (!launched) state = -1;                                  // no kernel for the shape: the launch path from now on
            return false;
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t spins = 1; load(&box->done[0]) != seq; ++spins) {
            if ((spins & 255) == 0) {
                // the wave may have left (idle / lifetime) between our look at the state and its last poll: start another one,
                // which finds the request waiting.  A wave that neither answers nor leaves within 2 s is a fault.
                if (load(&box->ctl[0]) == ISO_WAVE_EXITED && load(&box->done[0]) != seq) {
                    if (!start(launch)) return false;
                } else if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                    __atomic_store_n(&box->ctl[1], 1ull, __ATOMIC_RELEASE);
                    (void)hipStreamSynchronize(stream);
                    state = -1;
                    return false;
                }
            }
        }
        return true;
    }

    // ask the wave to leave and wait until it has (before the tables it reads go, or before a device-wide synchronise that
    // should not wait for the idle timeout); frees the box when `release`
    void stop(bool release)
    {
        if (!box) return;
        if (load(&box->ctl[0]) == ISO_WAVE_RUNNING) __atomic_store_n(&box->ctl[1], 1ull, __ATOMIC_RELEASE);
        (void)hipStreamSynchronize(stream);
        if (release) {
            (void)hipStreamDestroy(stream);
            (void)hipHostFree(box);
            *this = ResidentWave();
        }
    }

#ifdef ISO_MAILBOX_CLOCK
    // (variant builds) the wave's own time from seeing a request to its results (done[4], 100 MHz ticks), printed every 2000
    // calls; returns the number of calls when it printed, else 0
    unsigned long long clock(const char* label)
    {
        static unsigned long long calls = 0, ticks = 0;
        ticks += __atomic_load_n(&box->done[4], __ATOMIC_RELAXED);
        if (++calls % 2000 != 0) return 0;
        std::fprintf(stderr, "%s: %.2f us on the device per call (%llu calls)\n", label, ticks * 0.01 / (double)calls, calls);
        const unsigned long long n = calls;
        calls = ticks = 0;
        return n;
    }
#endif
};

}  // namespace iso
