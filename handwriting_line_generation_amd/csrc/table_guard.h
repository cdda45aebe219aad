// The bounds a kernel checks on an entry of a device-resident table before it reads or writes through it - the second line of defence
// behind the host validation in ops. This is the ONE place they are written: fg_mask.hip, lines_out.hip, line_store.hip, store_warp.hip and
// stretch.hip call these predicates (further conditions of a kernel - alignment of a width, a range of T_out - are conjoined there).
//
// They hold for ANY 64-bit offset: no sum of an offset and a size is ever formed (off + H * w wraps for an offset near 2^63 and lets the
// entry through); the size is compared with what is left behind the offset, `bytes - off`, which cannot overflow once 0 <= off <= bytes.
//
// Plain C++, no HIP include: a stand-alone host program includes this file and runs the predicates under a sanitizer
// (tests/test_table_guards_cpu.py); oracle/table_cases.py restates them in unbounded integers.
#pragma once

#if defined(__HIPCC__)
#define HWG_TG_FN __host__ __device__ inline
#else
#define HWG_TG_FN inline
#endif

// the row-major H x w picture at byte `off` lies inside a pool of `pixel_bytes` bytes (H >= 1 is checked by every entry point before the
// launch and again here; a pool that is stated negative holds nothing: 0 <= off <= pixel_bytes fails for it)
HWG_TG_FN bool hwg_line_in_pool(long long off, int w, int H, long long pixel_bytes) {
  return w >= 1 && H >= 1 && off >= 0 && off <= pixel_bytes && (long long)H * (long long)w <= pixel_bytes - off;
}

// the block of n elements at element `off` lies inside a buffer of `elems` elements and starts at a multiple of 4 (16-byte stores of floats)
HWG_TG_FN bool hwg_block_in_buffer(long long off, long long n, long long elems) {
  return n >= 0 && off >= 0 && (off & 3) == 0 && off <= elems && n <= elems - off;
}
