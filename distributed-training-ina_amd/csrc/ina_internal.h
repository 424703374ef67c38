// ina_internal.h -- shared between the libina.so translation units (not installed): the
// cross-source declarations, then the one copy of the small host helpers every entry point
// uses (stream cast, alignment and scale checks, grids, worker-pointer packs, launch check).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>

#include "ina.h"

namespace ina {

// W device pointers passed by value in the kernel arguments (512 B at W_max = 64)
template <typename T>
struct PtrPack {
    const T* p[INA_MAX_WORKERS];
};

int set_error(int code, const char* fmt, const char* detail);
int set_h2d_streams(int v);   // ina_host.cpp
int set_zero_copy(int v);     // ina_host.cpp
int sum_reduce_i32_impl(const int32_t* const* bufs, int W, int32_t* out, size_t n, ina_stream_t stream,
                        bool host);   // ina_kernels.hip
// ina_switch.hip: the switch keys of ina_set_tuning (9-13, 15, 17-21; the table g_switch_keys);
// INA_EINVAL for a key that is not the switch's or a value the key refuses
int set_switch_tuning(int key, int value);
int ew_grid_cap();            // ina_kernels.hip: grid cap of the elementwise kernels (tuning key 14)
int default_grid_cap();       // ina_kernels.hip: grid cap of the default-cap kernels (tuning key 0)
int stream_grid_cap();        // ina_kernels.hip: grid cap of the flat packet kernels (tuning key 4)
int combine_ina_grid_cap();   // ina_kernels.hip: grid cap of the INA combines, blk one included (tuning key 6)
// ina_blk.hip: ina_scale_for's rule for `degree` summands at `bits` (16 or 32): lim = (2^(bits-1) - 1) /
// degree - round, INA_EINVAL when it is not positive.  round: what one quantised value can gain by
// rounding -- 1/2 to nearest, 1 stochastically (ina_scale_for_sr's rule, include/ina_pkt_sr.h)
int scale_lim(int degree, int bits, double& lim, double round = 0.5);
// ina_blk.hip: the block-scaled calls' checks of V (>= 1) and of mode / degree / kblk (lim as above
// under INA_BLK_AUTO with scale_lim's round, else 1)
int check_v(int V);
int check_mode(int mode, const int8_t* kblk, int degree, int bits, double& lim, double round = 0.5);
// ina_blk.hip: where a block kernel's k comes from -- the call's one k (the error-feedback calls only),
// kblk[block] read, or the block's max |value| in the launch with kblk[block] written
enum { K_GLOBAL, K_GIVEN, K_AUTO };
// ina_blk.hip: the error-feedback launches (include/ina_ef.h; ina_ef.hip checks the arguments).  One
// bucket quantised: x is fp32 (xtype 0) or INA_X16_*, q int32 or int16 (bits); V is the block of
// K_GIVEN / K_AUTO, the slot of the int16 flags under K_GLOBAL (256 for int32 out).  The fields
// ina_ef.hip's initialisers leave out are zero.
struct EfQuant {
    const void* x;
    int xtype;
    const float* base;     // may be null
    float* resid;          // read, then written
    void* q;
    int bits;
    size_t n;
    int km;
    int k;                 // K_GLOBAL
    int8_t* kblk;          // K_GIVEN: read; K_AUTO: written
    double lim;            // K_AUTO
    int V;
    uint8_t* ovf;          // int16 out: may be null
    bool wire;             // include/ina_shard_ef.h: q holds int32 wire words q16 + (sat << 22); fp32 x,
                           // no base, bits 32, K_GLOBAL or K_GIVEN
};
int ef_quantize(const EfQuant& c, ina_stream_t stream);
// the scales alone over |(xs[w] - base) + rs[w]|; aligned: every xs[w] and rs[w] is 16-byte aligned
int ef_block_scales(const PtrPack<float>& xs, const PtrPack<float>& rs, int W, bool aligned, const float* base,
                    size_t n, int V, double lim, int8_t* kblk, ina_stream_t stream);
int check_x16_type(int xtype);   // ina_x16.hip: INA_OK for INA_X16_BF16 / INA_X16_F16, else INA_EINVAL
// checked builds (INA_STORE_CHECK, ina_device.h): each source's stream_store contract
// violations since the last read, cleared by the read
unsigned long long store_violations_kernels();   // ina_kernels.hip
unsigned long long store_violations_shard();     // ina_shard.hip
unsigned long long store_violations_switch();    // ina_switch.hip
unsigned long long store_violations_x16();       // ina_x16.hip
unsigned long long store_violations_blk();       // ina_blk.hip
unsigned long long store_violations_sr();        // ina_sr.hip
unsigned long long store_violations_reduce_sr(); // ina_reduce_sr.hip
// ina_kernels.hip: ina_scale_for with `round` for its 1/2 -- the largest k in [-126, 127] with
// W * (absmax * 2^k + round) <= 2^(bits-1) - 1; ina_scale_for's refusals
int scale_for_round(float absmax, int W, int bits, double round, int* k_out);

// ---------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------
constexpr int kHostBlock = 256;   // threads per workgroup of every kernel these grids are for

inline hipStream_t hs(ina_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// 256-thread workgroups covering `items`, at most `cap` (the kernels grid-stride beyond), at least 1
inline unsigned grid_of(size_t items, int cap) {
    size_t g = (items + kHostBlock - 1) / kHostBlock;
    if (g > (size_t)cap) g = (size_t)cap;
    return g ? (unsigned)g : 1u;
}
// the same with `per_thread` items a thread, under the default cap (tuning key 0) unless overridden
inline unsigned grid_for(size_t work_items, int per_thread, int cap_override = 0) {
    size_t per_block = (size_t)kHostBlock * (size_t)per_thread;
    size_t blocks = (work_items + per_block - 1) / per_block;
    size_t cap = (size_t)(cap_override > 0 ? cap_override : default_grid_cap());
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    return (unsigned)blocks;
}

// log2 of a power of two, -1 for anything else
inline int log2_exact(uint32_t v) {
    if (v == 0 || (v & (v - 1))) return -1;
    int s = 0;
    while ((1u << s) < v) ++s;
    return s;
}

// the block sizes of the block-scaled vector paths (a power of two in [8, 256]: a block is V/4
// adjacent lanes of one wave); shift = log2(V) - 2
inline bool vec_v(int V, int& shift) {
    if (V < 8 || V > 256 || log2_exact((uint32_t)V) < 0) return false;
    shift = log2_exact((uint32_t)V) - 2;
    return true;
}

inline int check_k(int k) {
    if (k < -126 || k > 127) return set_error(INA_EINVAL, "k out of range [-126,127]%s", "");
    return INA_OK;
}

// after a launch: INA_OK, or INA_EHIP with "<what>: <the runtime's error string>"
inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return INA_OK;
    return set_error(INA_EHIP, "%s", (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

// the W worker pointers into a pack; B = void: untyped 16-bit buffers (include/ina_x16.h), refused
// unless 2-byte aligned
template <typename T, typename B>
int fill_pack(PtrPack<T>& pk, const B* const* bufs, int W, bool& all_aligned) {
    if (!bufs || W < 1 || W > INA_MAX_WORKERS) return set_error(INA_EINVAL, "W must be in [1, %s]", "64");
    all_aligned = true;
    for (int w = 0; w < W; ++w) {
        if (!bufs[w]) return set_error(INA_EINVAL, "null worker buffer%s", "");
        if constexpr (std::is_void_v<B>) {
            if ((uintptr_t)bufs[w] & 1u) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
        }
        pk.p[w] = static_cast<const T*>(bufs[w]);
        all_aligned &= aligned16(bufs[w]);
    }
    for (int w = W; w < INA_MAX_WORKERS; ++w) pk.p[w] = nullptr;
    return INA_OK;
}

}  // namespace ina

extern "C" int ina_set_tuning(int key, int value);
