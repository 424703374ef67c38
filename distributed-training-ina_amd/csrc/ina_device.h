// ina_device.h -- device-side helpers shared by the HIP sources of libina.so.
#pragma once
#include <hip/hip_runtime.h>

#include "ina.h"

namespace ina {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// Streaming stores of the one-pass reduce and elementwise kernels: stores with the sc1
// cache-policy bit (write-through at system scope), so a launch leaves no dirty lines for the next
// dependent launch's boundary to drain (MI355X_MICROARCH.md: a boundary costs + B / 6 TB/s
// when the predecessor leaves B bytes dirty).  The headline reduce, interleaved on two
// boxes (tools/lab/store_policy_lab.py, profiles/r03/lab/store_policy_lab*.log): back to
// back 151.7 -> 150.9 and 149.2 -> 147.1 us, single launches 157.2 -> 153.1 and
// 152.7 -> 148.5 us against the non-temporal (nt) stores of rounds 1-2; default-policy stores
// 155.8-156.4.
//
// The sc1 store is a compiler builtin (`__builtin_amdgcn_raw_buffer_store_b*`, aux bit 4 =
// SC1 on gfx950), never inline asm: the compiler then owns the store's wait states and
// hazards (round 3's asm store needed a hand-placed s_nop -- a VALU overwrite of the data
// VGPRs of a >8-byte store -- and gave wrong W = 16 sums without it).  A buffer store needs
// a wave-uniform base: the wave's first active lane's address (readfirstlane) is the
// resource base and every lane stores at its byte distance from it.
// CONTRACT: at every call site a lane's address is >= the first active lane's (lanes
// store at wave_base + lane * sizeof(T), or at rising packet / slot positions), so the
// distance is small and positive.  Every caller in csrc/ keeps it (a lane below the first
// one would fall outside the resource and its store would be dropped -- which the parity
// tests of every kernel would see).  A per-store check with an ordinary-store fallback
// measured 4-7 % slower on the streaming kernels and 2.3x on the int16 reduce (the branch
// split the unrolled loop and doubled its registers; profiles/r04/lab/store_builtin_lab.log).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "stream_store's SC1 cache-policy bit (aux bit 4) is the gfx942 / gfx950 encoding"
#endif
// buffer resource word 3 for a raw (stride 0, untyped) gfx9 buffer: 32-bit data format
constexpr int kRawBufferWord3 = 0x00020000;
constexpr int kAuxSC1 = 16;
// INA_STORE_CHECK = 1 (checked builds: make BUILD=build_chk OUT=... EXTRA=-DINA_STORE_CHECK=1):
// every stream_store verifies the CONTRACT above -- its lane's distance from the wave's base is
// in [0, 2^31 - sizeof(T)] -- and counts each store that breaks it in a per-source device
// counter (ina_store_check_violations reads and clears them; tests/test_gpu_store_views.py and
// the conftest hook of a checked run assert zero).  Counted, not trapped: a trap is a GPU fault,
// and on this pool a faulting kernel can take the machine's GPUs down with it.
#ifndef INA_STORE_CHECK
#define INA_STORE_CHECK 0
#endif
#if INA_STORE_CHECK
static __device__ unsigned long long g_store_violations;   // one per source file
// host: this source's count since the last read, cleared by the read
static inline unsigned long long take_store_violations() {
    unsigned long long v = 0, z = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_store_violations), sizeof(v)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_store_violations), &z, sizeof(z)) != hipSuccess)
        return ~0ull;                                  // unreadable: report as a violation
    return v;
}
#endif
template <typename T>
__device__ __forceinline__ void stream_store(T v, T* p) {
    static_assert(sizeof(T) == 16 || sizeof(T) == 8 || sizeof(T) == 4, "16, 8 or 4-byte stores");
    const uint64_t a = (uint64_t)(uintptr_t)p;
    // (readfirstlane returns int: each half goes through uint32_t, or the low half's bit 31
    // would sign-extend into the high half)
    const uint64_t a0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t d = (uint32_t)(a - a0);
#if INA_STORE_CHECK
    const int64_t dist = (int64_t)(a - a0);
    if (dist < 0 || dist > (int64_t)0x7FFFFFFF - (int64_t)sizeof(T))
        atomicAdd(&g_store_violations, 1ull);
#endif
    __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)a0, 0, 0x7FFFFFFF, kRawBufferWord3);
    if constexpr (sizeof(T) == 16)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, (int)d, 0, kAuxSC1);
    else if constexpr (sizeof(T) == 8)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, v), r, (int)d, 0, kAuxSC1);
    else
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, (int)d, 0, kAuxSC1);
}

// Packet kernels (pack / unpack of NGA rows) keep non-temporal stores: their rows are the
// next launch's input (the switch, the sender), and write-through made the fused worker
// pack 9 % slower in the packet path (54.7 -> 59.6 us per launch beside the switch,
// profiles/r03/lab/path_store_lab.log).
template <typename T>
__device__ __forceinline__ void packet_store(T v, T* p) {
    __builtin_nontemporal_store(v, p);
}


// ---------------------------------------------------------------------------
// quantiser (build-defined, see include/ina.h): sat(rne(x * 2^k)), NaN -> 0
// ---------------------------------------------------------------------------
// (each quantiser is its rounding, rintf(x * s), then the clamp / NaN handling of the rounded y: the
// *_of functions, which the stochastic-rounding kernels of ina_sr.hip run on their own y)
__device__ __forceinline__ int32_t q32_of(float y) {
    int32_t r = (int32_t)y;                         // in-range lanes only are selected
    r = (y >= 2147483648.0f) ? INT32_MAX : r;
    r = (y < -2147483648.0f) ? INT32_MIN : r;
    return (y != y) ? 0 : r;
}
__device__ __forceinline__ int32_t q32(float x, float s) { return q32_of(__builtin_rintf(x * s)); }

// returns the int16 value widened to int32; *sat |= clamped-or-NaN
__device__ __forceinline__ int32_t q16_of(float y, bool& sat) {
    // one v_med3_f32 clamps; a clamped value, +-inf or NaN differs from y
    const float c = __builtin_amdgcn_fmed3f(y, -32768.0f, 32767.0f);
    sat |= !(c == y);
    return (y != y) ? 0 : (int32_t)c;
}
__device__ __forceinline__ int32_t q16(float x, float s, bool& sat) { return q16_of(__builtin_rintf(x * s), sat); }

__device__ __forceinline__ int32_t sat16(int32_t a, bool& sat) {
    bool hi = a > 32767, lo = a < -32768;
    sat |= hi | lo;
    return hi ? 32767 : (lo ? -32768 : a);
}

// the word of the sharded int16 wire (include/ina.h; ina_shard.hip): the quantiser of
// ina_quantize_f32_i16_sat, sat16(rne(x * 2^k)), NaN -> 0 (flagged), with the saturation bit above
// it -- q16 + (sat << 22).  The one copy: the wire quantisers of ina_shard.hip and their
// error-feedback siblings (the kernels of ina_blk.hip) run it.
constexpr int kWireShift = INA_I16_WIRE_SHIFT;   // 22
__device__ __forceinline__ int32_t q16w_of(float y) {
    const float c = __builtin_amdgcn_fmed3f(y, -32768.0f, 32767.0f);   // one v_med3_f32
    const int32_t v = (y != y) ? 0 : (int32_t)c;
    const int32_t sat = !(c == y);               // clamped, +-inf or NaN
    return v + (sat << kWireShift);
}
__device__ __forceinline__ int32_t q16w(float x, float s) { return q16w_of(__builtin_rintf(x * s)); }
// q16 back out of one rank's word: its low 22 bits, sign-extended (|q16| <= 2^15, sat is 0 or 1)
__device__ __forceinline__ int32_t wire_q16(int32_t w) {
    return (int32_t)((uint32_t)w << (32 - kWireShift)) >> (32 - kWireShift);
}

// ---------------------------------------------------------------------------
// per-slot overflow flags: thread t owns 8 consecutive values; a slot of V values
// (V % 8 == 0, V/8 a power of two <= 64) is V/8 adjacent lanes of one wave.  The
// group's first lane writes the slot flag from a wave ballot -- one writer per slot,
// no atomics, no pre-zeroing.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void write_slot_flags8(unsigned long long m, bool active, size_t elem0,
                                                  int V, int lanes_per_slot,
                                                  uint8_t* __restrict__ ovf) {
    int lane = threadIdx.x & 63;
    int g0 = lane & ~(lanes_per_slot - 1);
    unsigned long long gm = (lanes_per_slot == 64) ? ~0ull : (((1ull << lanes_per_slot) - 1ull) << g0);
    if (active && (lane & (lanes_per_slot - 1)) == 0) ovf[elem0 / (size_t)V] = (m & gm) ? 1 : 0;
}

// the same for the split layout of the int16 kernels (ina_kernels.hip: a wave owns
// 512 values, lane l holds 4 at 4l of each 256-value half): a slot is V/4 adjacent lanes of one
// half, or both halves at V = 512
__device__ __forceinline__ void write_slot_flags_split(unsigned long long ma, unsigned long long mb,
                                                       size_t eA, size_t eB, size_t n, int V,
                                                       uint8_t* __restrict__ ovf) {
    if (V >= 512) {
        write_slot_flags8(ma | mb, eA < n, eA, V, 64, ovf);
    } else {
        write_slot_flags8(ma, eA < n, eA, V, V / 4, ovf);
        write_slot_flags8(mb, eB < n, eB, V, V / 4, ovf);
    }
}

static inline bool slot_ballot_ok(int V) {
    if (V % 8) return false;
    int l = V / 8;
    return l >= 1 && l <= 64 && (l & (l - 1)) == 0;
}



// ---------------------------------------------------------------------------
// 16-bit float sources and targets (include/ina.h, INA_X16_BF16 / INA_X16_F16).  Widening is
// exact: bf16 is the top half of an fp32 word; fp16 goes through v_cvt_f32_f16, which keeps
// subnormals (the fp16 denormal mode is on by default).  Two values travel in one dword, the
// lower-addressed one in the low half.
// ---------------------------------------------------------------------------
typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <int XT>
__device__ __forceinline__ float widen16(uint16_t h) {
    static_assert(XT == 1 || XT == 2, "INA_X16_BF16 or INA_X16_F16");
    if constexpr (XT == 1) return __uint_as_float((uint32_t)h << 16);
    else return (float)__builtin_bit_cast(_Float16, h);
}
template <int XT>
__device__ __forceinline__ f32x4_t widen16x4(u32x2_t v) {
    if constexpr (XT == 1)
        return f32x4_t{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u),
                       __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u)};
    else
        return f32x4_t{widen16<XT>((uint16_t)(v.x & 0xFFFFu)), widen16<XT>((uint16_t)(v.x >> 16)),
                       widen16<XT>((uint16_t)(v.y & 0xFFFFu)), widen16<XT>((uint16_t)(v.y >> 16))};
}
// fp32 -> 16-bit, one rounding to nearest even.  fp16: v_cvt_f16_f32 (overflow to +-inf,
// subnormal results produced), never the packed round-toward-zero convert.
template <int XT>
__device__ __forceinline__ uint32_t rne16(float f) {
    static_assert(XT == 1 || XT == 2, "INA_X16_BF16 or INA_X16_F16");
    if constexpr (XT == 1) {
        const uint32_t u = __float_as_uint(f);
        const uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
        return (f != f) ? ((u >> 16) | 0x0040u) : r;
    } else {
        return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    }
}
template <int XT>
__device__ __forceinline__ uint32_t rne16x2(float lo, float hi) {
    return rne16<XT>(lo) | (rne16<XT>(hi) << 16);
}

// ---------------------------------------------------------------------------
// per-block scales (include/ina_blk.h): shared by ina_blk.hip and the block-scaled packet
// kernels of ina_kernels.hip
// ---------------------------------------------------------------------------
// a given scale: -127 / -128 read as -126
__device__ __forceinline__ int rd_k(const int8_t* __restrict__ kblk, size_t s) {
    const int k = kblk[s];
    return k < -126 ? -126 : k;
}
// 2^k for k in [-127, 127], built from its bits: 2^-127 is the subnormal 0x00400000 (ldexpf(1, -127)),
// which an exp2 / division would flush or round
__device__ __forceinline__ float pow2f(int k) {
    return __uint_as_float(k >= -126 ? (uint32_t)(k + 127) << 23 : 0x00400000u);
}
// |d| as its bit pattern, NaN -> 0
__device__ __forceinline__ uint32_t absbits(float d) {
    const uint32_t u = __float_as_uint(d) & 0x7FFFFFFFu;
    return u > 0x7F800000u ? 0u : u;
}
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t fold4(uint32_t m, f32x4_t a) {
    return umax(umax(m, absbits(a.x)), umax(umax(absbits(a.y), absbits(a.z)), absbits(a.w)));
}

// ina_scale_for(amax, degree, bits) for amax given as its bits and lim = (2^(bits-1) - 1) / degree
// - 1/2 as the host computed it: the largest k in [-126, 127] with amax * 2^k <= lim (-126 if
// none).  amax = ma * 2^ea, lim = ml * 2^el with ma, ml in [1, 2): k = el - ea when ma <= ml, else
// el - ea - 1 -- exponents and mantissas compared as integers, so the answer is the host's exact
// double comparison for every fp32 amax (an fp32 mantissa, subnormal ones included, converts to
// double exactly).
__device__ __forceinline__ int scale_of(uint32_t u, double lim) {
    if (u == 0u) return 127;
    if (u >= 0x7F800000u) return -126;
    const uint32_t e = u >> 23, m = u & 0x7FFFFFu;
    const uint64_t d = (uint64_t)__double_as_longlong((double)(e ? (m | 0x800000u) : m));   // exact
    const int ea = (int)(d >> 52) - 1023 + (int)(e ? e : 1u) - 150;
    const uint64_t l = (uint64_t)__double_as_longlong(lim);
    const int el = (int)(l >> 52) - 1023;
    const uint64_t mant = (1ull << 52) - 1ull;
    int k = el - ea - ((d & mant) > (l & mant) ? 1 : 0);
    return k < -126 ? -126 : (k > 127 ? 127 : k);
}

// max over the `lanes` (a power of two <= 64, wave-uniform) adjacent lanes of a group; every
// lane of the wave must reach it
__device__ __forceinline__ uint32_t group_max(uint32_t m, int lanes) {
    for (int off = 1; off < lanes; off <<= 1) m = umax(m, (uint32_t)__shfl_xor((int)m, off, 64));
    return m;
}

}  // namespace ina
