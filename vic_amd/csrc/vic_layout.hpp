// vic_layout.hpp — layout of the two per-HRU tables the rounds of the finite-difference pipeline exchange: the item blocks
// the opening stage hands to the profile-solve kernels ("pin") and the solution records those hand to the evaluation kernel and
// the closing stage ("pout").  Plain index arithmetic, host and device: every reader and writer goes through these
// accessors, nothing indexes either table by hand (tests/test_round_layout.py checks them on the host).
//
// Both tables are laid out for the 64-byte sector HBM traffic is counted in: every HRU's entry starts on a sector boundary
// (strides are multiples of 8 words, the bases come from hipMalloc, which aligns to 256 bytes), and what one access needs
// sits together at the entry's start.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vic {

constexpr int SECTOR_WORDS = 8;        // 64 bytes of doubles
__host__ __device__ constexpr int sector_round(int words) { return (words + SECTOR_WORDS - 1) / SECTOR_WORDS * SECTOR_WORDS; }

// ------------------------------------------------------------------------------------------------
// Item block: what a profile solve of one HRU reads.
//   [0]                      header: frozen_on (1.0 / 0.0)
//   [1 .. Nn]                the start column: T0 of nodes 0 .. Nn-1 (node 0's is replaced by the trial surface temperature)
//   [1 + Nn ..]              the node records of nodes 1 .. Nn-1, PREC words each (PR_*, vic_surface.hpp); the bottom node's
//                            is last, and is written and read only with NOFLUX
// so without NOFLUX a solve reads the contiguous prefix header + column + interior records and nothing else.
// ------------------------------------------------------------------------------------------------
constexpr int PREC = 10;
enum { PR_AT0 = 0, PR_B, PR_C, PR_D, PR_EI, PR_S, PR_G, PR_Y, PR_EMOIST, PR_EMM };

__host__ __device__ constexpr int item_header() { return 0; }
__host__ __device__ constexpr int item_t0(int j) { return 1 + j; }
__host__ __device__ constexpr int item_rec(int Nn, int j) { return 1 + Nn + (j - 1) * PREC; }      // 1 <= j <= Nn - 1
__host__ __device__ constexpr int item_words(int Nn) { return 1 + Nn + (Nn - 1) * PREC; }
__host__ __device__ constexpr int item_stride(int Nn) { return sector_round(item_words(Nn)); }
// the words a solve without NOFLUX fetches
__host__ __device__ constexpr int item_prefix_words(int Nn) { return item_rec(Nn, Nn - 1); }
// An HRU's block.  It starts on a 16-byte boundary (on a sector boundary in fact, but 16 bytes are what the register-resident
// kernel's paired loads rely on, and all a host allocator promises the host-emulation build): the compiler may merge the
// loads of two neighbouring words at an even offset into one access.
template <class T>
__host__ __device__ inline T* item_block(T* pin, size_t hru, int Nn) {
  return static_cast<T*>(__builtin_assume_aligned(pin + hru * (size_t)item_stride(Nn), 16));
}

// ------------------------------------------------------------------------------------------------
// Solution record of one profile solve; every HRU keeps the records of its last two solves, one after the other.
//   [0]                      T of node 0 = the trial surface temperature the solve was made for (no sweep changes node 0): the
//                            key the final evaluation looks the solve up by.  NaN: no solve on record.
//   [1]                      flag word {fbmask | ok << NodeBound<NN>::ok_bit}
//   [2 .. Nn]                T of nodes 1 .. Nn-1
//   [Nn + 1 ..]              int fall-back counts [Nn], two to a word
// An evaluation of the iteration reads words 0 .. 3 (key, flags, T1, T2): the record's first sector.
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int rec_key() { return 0; }
__host__ __device__ constexpr int rec_flag() { return 1; }
__host__ __device__ constexpr int rec_t(int j) { return j == 0 ? 0 : j + 1; }
__host__ __device__ constexpr int rec_cnt(int Nn) { return Nn + 1; }                    // word offset of the int counters
__host__ __device__ constexpr int rec_words(int Nn) { return Nn + 1 + (Nn + 1) / 2; }
__host__ __device__ constexpr int pout_stride(int Nn) { return sector_round(rec_words(Nn)); }
__host__ __device__ constexpr int pout_hru_stride(int Nn) { return 2 * pout_stride(Nn); }
template <class T>
__host__ __device__ inline T* pout_rec(T* pout, size_t hru, int Nn, int slot) {
  return pout + hru * (size_t)pout_hru_stride(Nn) + (size_t)slot * pout_stride(Nn);
}

static_assert(item_stride(10) % SECTOR_WORDS == 0 && item_stride(50) % SECTOR_WORDS == 0 && pout_stride(10) % SECTOR_WORDS == 0
              && pout_stride(24) % SECTOR_WORDS == 0 && pout_stride(50) % SECTOR_WORDS == 0, "entries start on sector boundaries");
static_assert(rec_key() < SECTOR_WORDS && rec_flag() < SECTOR_WORDS && rec_t(1) < SECTOR_WORDS && rec_t(2) < SECTOR_WORDS,
              "an evaluation of the iteration reads one sector of the record");
static_assert(pout_hru_stride(10) == 32 && rec_words(10) == pout_stride(10), "10 nodes: a solve writes two full sectors, 256 bytes per HRU");
static_assert(item_prefix_words(10) == 91 && item_stride(10) == 104, "10 nodes: a solve fetches 91 words in 12 of the block's 13 sectors");
static_assert(SECTOR_WORDS * sizeof(double) % 16 == 0, "a sector-aligned block is 16-byte aligned (item_block)");

}  // namespace vic
