/*
 * ina_x16.h -- the bf16 / fp16 entry points of libina.so.  Included by ina.h (after the
 * packet types these declarations use); the semantics are stated there, under
 * "bf16 / fp16 gradients".  Do not include this file on its own.
 */
#ifndef INA_X16_H
#define INA_X16_H

#ifndef INA_H
#error "include ina.h, which includes ina_x16.h"
#endif

#define INA_X16_BF16 1
#define INA_X16_F16 2
/* ina_quantize_f32_i32 / ina_quantize_f32_i16_sat */
int ina_quantize_x16_i32(const void* x, int xtype, int32_t* q, size_t n, int k, ina_stream_t stream);
int ina_quantize_x16_i16_sat(const void* x, int xtype, int16_t* q, size_t n, int k, int V,
                             uint8_t* overflow_per_slot, ina_stream_t stream);
/* ina_quantize_reduce_f32_i32 / ina_quantize_reduce_f32_i16_sat: all W buffers of one xtype */
int ina_quantize_reduce_x16_i32(const void* const* bufs, int xtype, int W, int32_t* out, size_t n,
                                int k, ina_stream_t stream);
int ina_quantize_reduce_x16_i16_sat(const void* const* bufs, int xtype, int W, int16_t* out, size_t n,
                                    int k, int V, uint8_t* overflow_per_slot, ina_stream_t stream);
/* ina_absmax_multi_f32 (W = 1 is the single-bucket form, ina_absmax_f32) */
int ina_absmax_multi_x16(const void* const* xs, int xtype, int W, const float* base, size_t n,
                         float* out_dev, ina_stream_t stream);
/* ina_quantize_pack_nga_desc (packed rows; desc may be NULL) */
int ina_quantize_pack_nga_x16_desc(const void* x, int xtype, const float* base, size_t n, int k,
                                   const ina_nga_params_t* prm, uint8_t* pkts, size_t stride,
                                   ina_nga_desc_t* desc, ina_stream_t stream);
/* ina_quantize_pack_nga_multi_split (split rows; base read once per 8 workers) */
int ina_quantize_pack_nga_multi_split_x16(const void* const* x, int xtype, int W, const float* base,
                                          size_t n, int k, const ina_nga_params_t* prm,
                                          uint8_t* const* hdr, uint8_t* const* pay,
                                          ina_nga_desc_t* const* desc, ina_stream_t stream);
/* ina_dequantize_i32_f32 / ina_dequantize_i16_f32 into a 16-bit buffer of type ytype */
int ina_dequantize_i32_x16(const int32_t* s, void* y, int ytype, size_t n, int k, ina_stream_t stream);
int ina_dequantize_i16_x16(const int16_t* s, void* y, int ytype, size_t n, int k, ina_stream_t stream);

#endif /* INA_X16_H */
