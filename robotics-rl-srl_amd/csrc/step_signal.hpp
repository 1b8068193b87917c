// step_signal.hpp — the two device -> host hand-offs of the per-step API, in one place: the memory layout both ends address, the device
// side of the protocol (called by mobile.hip's and kuka_tree_kernels.hpp's kernels) and the two maps from workgroups to eighths of the
// grid.  The host side is api.hip (persist_launch, host_step_begin, host_step_finish).  Not part of the ABI.
//
// PERSISTENT STEPPING (srlhip_set_persistent): the per-step API without a launch per step.  ONE launch of the rollout kernel stays
// resident — every wavefront keeps its envs' state in registers — and takes its steps from the host through mapped memory: the host
// writes the actions, then a new sequence number; every wavefront fetches it, steps and writes its outputs, and
// the last wavefront of each EIGHTH of the grid to arrive reports: the host polls 8 `done` words.  The kernel PARKS (writes the state
// back and exits) when told to (any other API call on the handle) or when no step arrived for park_us.
//
// Where the outputs go.  Neither way of writing them to the host's mapped planes directly works from 1024 independent wavefronts: a
// plain store stays in the XCD's L2 until a write-back (measured: the host saw the previous step's observations; a release fence per
// wavefront writes back the whole L2 — generator states, spills — 1024 times per step: 121 us), a system-scope store of 1-12 bytes
// crosses PCIe as its own serialised transaction (~40 ns each, 20 k per step: 835 us).  Hence the eighths: workgroup b runs on XCD
// b mod 8 and every XCD has its own L2, so an eighth of the grid that IS one XCD (verified behind a start barrier) writes its outputs
// STRAIGHT to the mapped planes by plain stores — they stay in that L2 — and its last arriver writes the L2 back ONCE, by one
// system-scope release: that write-back is the transfer.  On any other placement the outputs go to a staging copy in device memory by
// agent-scope (write-through) stores, "written through" = the store counter reaching 0, and the last arriver copies its eighth's range
// out (Kuka: kuka_tree_kernels.hpp persist_copy), or they are written through to the host (MobileRobot: slow, correct).
//
// EARLY COMPLETION SIGNAL of a single-step launch on a host-pointer handle (host_step_begin arms it: PersistArgs::done set): the host
// does not wait for the kernel to END (exit stores of ~40 state planes, the completion signal, the stream synchronisation's wake-up) —
// the step's outputs are plain stores to its mapped planes in the XCD's L2, and the last wavefront of each eighth of the grid writes
// that L2 back and reports, as in persistent stepping.  Which XCD is immaterial — a second kernel running beside this one shifts the
// round-robin — as long as the eighth's workgroups all sit on the SAME one: hence the eighth's XCD tag.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace srl {

struct PersistArgs {
    const uint32_t *seq, *stop;     // host-written (mapped, coherent): sequence number of the newest step; 1 = park now
    uint32_t *parked;               // device-written: workgroup 0 decided to park (the host must synchronise and relaunch)
    uint32_t *done;                 // device-written [8]: sequence number of the last step that eighth of the workgroups finished
    uint32_t *relay;                // device memory [8 x stride]: workgroup 0's token for the others (a sequence number, or kPersistPark)
    uint32_t *count;                // device memory [8 x stride]: arrivals per eighth of the workgroups, never reset while resident
    uint32_t *ctrl;                 // device memory: [0] workgroups registered | XCD mismatches << 16, [stride] the start barrier's verdict
    const uint32_t *stage;          // device memory: the staging copy of the step's output planes (same layout as the host's), dword view
    uint32_t *host_out;             // the host's mapped output planes, dword view; reward / done planes start rew_dw / done_dw dwords in
    uint32_t rew_dw, done_dw;
    uint32_t start_seq, spin_limit; // (single-step signal: start_seq = the step's sequence number)
    uint32_t force_staged;          // SRLHIP_PERSIST_STAGED=1: the staging copy + copier even where the direct form is valid (tests run both)
};
constexpr int kPersistWordStride = 64;         // (uint32 words: 256 bytes — one memory channel — between two relay / counter words)
constexpr uint32_t kPersistPark = 0xffffffffu;

// ---- layout ------------------------------------------------------------------------------------------------------------------------
// The host block: mapped, coherent.  (seq, stop) are one aligned 8-byte word: ONE PCIe read per poll of workgroup 0.
constexpr int kDoneResident = 0, kDoneStep = 8;            // done[0..7]: the resident kernel's eighths; done[8..15]: the single-step signal's
struct PersistHost { volatile uint32_t seq, stop, parked; volatile uint32_t pad[13]; volatile uint32_t done[16]; };
static_assert(offsetof(PersistHost, seq) == 0 && offsetof(PersistHost, stop) == 4 && offsetof(PersistHost, parked) == 8, "PersistHost: (seq, stop) is the 8-byte word the device polls");
static_assert(offsetof(PersistHost, done) == 16 * 4 && sizeof(PersistHost) == 32 * 4, "PersistHost: the done words have a 64-byte line to themselves");

// The device words (uint32; Handle::persist_relay): eight words of a kind lie kPersistWordStride apart.
constexpr int kWordRelay = 0;                                    // x8: workgroup 0's token; a poller reads the word of its blockIdx % 8
constexpr int kWordCount = 8 * kPersistWordStride;               // x8: the resident kernel's arrival counter per eighth
constexpr int kWordCtrl = 16 * kPersistWordStride;               // workgroups registered | XCD mismatches << 16
constexpr int kWordVerdict = 17 * kPersistWordStride;            // the start barrier's verdict
// (18, 19 x stride: RESERVED — a (re)launch of the resident kernel resets all of [kWordCount, kWordStepCount))
constexpr int kWordStepCount = 20 * kPersistWordStride;          // x8: the single-step signal's arrival counter, [+1] its XCD tag
constexpr int kWordStamps = 28 * kPersistWordStride;             // timeline build: 8 uint64 stamps per workgroup
constexpr int kStampsPerBlock = 8;
constexpr size_t signal_words(size_t blocks) { return kWordStamps + 2 * kStampsPerBlock * ((blocks + 7) / 8 * 8); }

enum class SignalKind { resident, single_step };
// `host`: the device's view of the PersistHost block; `words`: the device words
inline PersistArgs signal_args(SignalKind kind, void *host, uint32_t *words) {
    uint32_t *w = static_cast<uint32_t *>(host);
    PersistArgs a{};
    a.done = w + offsetof(PersistHost, done) / 4 + (kind == SignalKind::resident ? kDoneResident : kDoneStep);
    a.count = words + (kind == SignalKind::resident ? kWordCount : kWordStepCount);
    if (kind == SignalKind::single_step) return a;
    a.seq = w + offsetof(PersistHost, seq) / 4; a.stop = w + offsetof(PersistHost, stop) / 4; a.parked = w + offsetof(PersistHost, parked) / 4;
    a.relay = words + kWordRelay; a.ctrl = words + kWordCtrl;
    return a;
}

// ---- the eighths of a grid ------------------------------------------------------------------------------------------------------------
// Host and device must agree exactly on which eighths hold a real workgroup and how many units arrive in each, or step_wait waits for a
// word nobody writes.
// STRIDED (MobileRobot): eighth g = the workgroups b = g mod 8; arrivals are WAVEFRONTS with a live lane, `wpb` per full workgroup.
constexpr __host__ __device__ uint32_t strided_eighths(int blocks) { return blocks >= 8 ? 0xffu : (1u << blocks) - 1u; }
constexpr __host__ __device__ int strided_real(int g, int waves, int wpb) {
    int real = 0;
    for (int b = g; b * wpb < waves; b += 8) real += wpb < waves - b * wpb ? wpb : waves - b * wpb;
    return real;
}
// CONTIGUOUS (Kuka): eighth g = the workgroup range [g, g + 1) * per, per = ceil(blocks / 8) — the grid is 8 * per workgroups, the
// rollout kernel maps them to envs XCD by XCD; arrivals are real WORKGROUPS (one wavefront each).
constexpr __host__ __device__ int contiguous_per(int blocks) { return (blocks + 7) / 8; }
constexpr __host__ __device__ int contiguous_grid(int blocks) { return 8 * contiguous_per(blocks); }
constexpr __host__ __device__ uint32_t contiguous_eighths(int blocks) {
    uint32_t mask = 0;
    for (int g = 0; g < 8 && g * contiguous_per(blocks) < blocks; g++) mask |= 1u << g;
    return mask;
}
constexpr __host__ __device__ int contiguous_real(int g, int blocks, int per) {
    const int real = blocks - g * per;
    return real > per ? per : real;
}

namespace eighths_check {
constexpr int strided_total(int waves, int wpb) {
    int sum = 0;
    for (int g = 0; g < 8; g++) if ((strided_eighths((waves + wpb - 1) / wpb) >> g) & 1u) sum += strided_real(g, waves, wpb);
    return sum;
}
constexpr int contiguous_total(int blocks) {
    int sum = 0;
    for (int g = 0; g < 8; g++) if ((contiguous_eighths(blocks) >> g) & 1u) sum += contiguous_real(g, blocks, contiguous_per(blocks));
    return sum;
}
static_assert(strided_eighths(1) == 0x01 && strided_eighths(7) == 0x7f && strided_eighths(8) == 0xff && strided_eighths(9) == 0xff && strided_eighths(17) == 0xff, "strided mask");
static_assert(strided_real(0, 9, 1) == 2 && strided_real(1, 9, 1) == 1 && strided_real(0, 17, 1) == 3 && strided_real(1, 17, 1) == 2 && strided_real(7, 7, 1) == 0, "strided counts");
static_assert(strided_real(0, 17, 4) == 4 && strided_real(4, 17, 4) == 1 && strided_real(5, 17, 4) == 0 && strided_real(0, 33, 4) == 5, "strided counts, 4 wavefronts per workgroup");
static_assert(strided_total(1, 1) == 1 && strided_total(7, 1) == 7 && strided_total(8, 1) == 8 && strided_total(9, 1) == 9 && strided_total(17, 1) == 17, "strided: every workgroup arrives once");
static_assert(strided_total(1, 4) == 1 && strided_total(7, 4) == 7 && strided_total(8, 4) == 8 && strided_total(9, 4) == 9 && strided_total(17, 4) == 17 && strided_total(33, 4) == 33, "strided: every wavefront arrives once");
static_assert(contiguous_eighths(1) == 0x01 && contiguous_eighths(7) == 0x7f && contiguous_eighths(8) == 0xff && contiguous_eighths(9) == 0x1f && contiguous_eighths(17) == 0x3f && contiguous_eighths(1024) == 0xff, "contiguous mask");
static_assert(contiguous_per(9) == 2 && contiguous_real(0, 9, 2) == 2 && contiguous_real(3, 9, 2) == 2 && contiguous_real(4, 9, 2) == 1, "contiguous counts: 9 workgroups = 2, 2, 2, 2, 1");
static_assert(contiguous_per(17) == 3 && contiguous_real(4, 17, 3) == 3 && contiguous_real(5, 17, 3) == 2 && contiguous_real(7, 1024, 128) == 128, "contiguous counts");
static_assert(contiguous_total(1) == 1 && contiguous_total(7) == 7 && contiguous_total(8) == 8 && contiguous_total(9) == 9 && contiguous_total(17) == 17 && contiguous_total(1024) == 1024, "contiguous: every workgroup arrives once");
}  // namespace eighths_check

// ---- device side ----------------------------------------------------------------------------------------------------------------------
// Every function is called by the ONE lane that talks for its wavefront / workgroup (Kuka: threadIdx.x == 0 of a one-wavefront workgroup;
// MobileRobot: thread 0 of the workgroup at the start barrier and the token, a wavefront's first active lane at the arrival), except
// xcd_id and signal_writeback (whole wavefront).  How the token and the verdict reach the other lanes is the caller's business.
__device__ __forceinline__ uint32_t xcd_id() {
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return xcc;
}
__device__ __forceinline__ uint32_t *eighth_counter(uint32_t *count, int g) { return count + g * kPersistWordStride; }     // [+1]: its XCD tag

// Every workgroup of the resident kernel (the padding ones too) registers with the XCD it runs on.  One word: count | mismatches << 16.
__device__ __forceinline__ void persist_register(const PersistArgs &pa, uint32_t xcc) {
    __hip_atomic_fetch_add(pa.ctrl, 1u + (((xcc & 15u) != (blockIdx.x & 7u)) ? 0x10000u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The start barrier (workgroup 0 waits for gridDim.x registrations or `stop` and publishes the verdict in ctrl[kWordVerdict - kWordCtrl] —
// 1: every eighth sits on one XCD -> direct outputs; 2: not so (or force_staged) -> staged / written through; 3: told to stop while
// waiting -> everybody parks — the others wait for it) and the token fetch (workgroup 0, the one poller on the bus, polls the 8-byte
// (seq, stop) up to spin_limit times, writes `parked` and relays a sequence number or kPersistPark to the 8 relay words, 256 bytes =
// one memory channel apart; the others poll the word of their blockIdx % 8, ~128 pollers per word) stay written out in the two resident
// kernels: as force-inlined functions the same statements compiled to other scalar code there (the compiler simplifies a function on
// its own before it inlines it) and moved the kernels' spill counts (profiles/NOTES.md section AC).

// Arrive at an eighth's counter (the unit's outputs are written: the caller has waited for its store counter); true: this was the last of
// the eighth's `real` units.  The counter is never reset between steps: after k steps it stands at k * real.
__device__ __forceinline__ bool signal_arrive(uint32_t *cnt, int real, uint32_t k) {
    return __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == (uint32_t)real * k;
}
// The last arriver (whole wavefront) writes its L2 back ...
__device__ __forceinline__ void signal_writeback() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, ""); }
// ... and then its one lane posts the eighth's `done` word.  The resident kernel: the step's sequence number.
__device__ __forceinline__ void persist_post(const PersistArgs &pa, int g, uint32_t seq) {
    __hip_atomic_store(pa.done + g, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The single-step signal.  Before it arrives, a unit ORs its XCD's bit into the eighth's tag (and waits for that and its output stores).
__device__ __forceinline__ void step_signal_tag(uint32_t *cnt, uint32_t xcc) {
    __hip_atomic_fetch_or(cnt + 1, 1u << (xcc & 15u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The last arriver, after signal_writeback: the tag goes back to 0 for the next launch; one XCD: the write-back carried the whole
// eighth -> the sequence number; several: its complement (the host then waits for the kernel's end, where every L2 is written back).
__device__ __forceinline__ void step_signal_post(const PersistArgs &sig, uint32_t *cnt, int g) {
    const uint32_t seen = __hip_atomic_exchange(cnt + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sig.done + g, (seen & (seen - 1u)) ? ~sig.start_seq : sig.start_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace srl
