// crc8_dev.h -- the CRC-8 of DVB-S2 mode adaptation on the device, shared by the BBFRAME de-header and the BB framer. Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dvbs2 {

// remainder modulo x^8 + x^7 + x^6 + x^4 + x^2 + 1 (lib/bbdeheader_bb_impl.cc:55), one byte at a time: the register after a
// byte is the remainder of (register * x^8 + byte), i.e. table[register's contribution] folded with the incoming byte
__device__ __forceinline__ uint32_t crc8_step(uint32_t reg, uint32_t byte, const uint8_t* tab)
{
    // (reg * x^8 + byte) mod g = (reg * x^8 mod g) ^ byte  [deg(byte) < 8]; tab[r] = r * x^8 mod g
    return (uint32_t)tab[reg] ^ byte;
}
__device__ __forceinline__ void crc8_build(uint8_t* tab, int tid, int nthreads)
{
    for (int r = tid; r < 256; r += nthreads) {
        uint32_t v = (uint32_t)r << 8; // r * x^8, reduce the upper eight bits
        for (int b = 15; b >= 8; b--) if (v & (1u << b)) v ^= 0x1D5u << (b - 8);
        tab[r] = (uint8_t)v;
    }
}

} // namespace dvbs2
