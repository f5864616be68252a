// One of the emulator sources of the kernels that carry K1's parse (emu_raw.cpp, emu_sz.cpp, emu_update.cpp, emu_resize.cpp:
// K1_CARRIER_SOURCE) with the second statistics array readable as well (pim-compression_amd/csrc/snappy_kernels.hpp:
// g_alias_stats), as tests/emu/emu_k1_alias.cpp makes it for the product kernels: a library per carrier, built by
// tests/emu_k1_carriers_lib.py.  Test infrastructure only.
#include K1_CARRIER_SOURCE

extern "C" {

// the 16 entries of g_alias_stats, cleared by the read
void emu_alias_stats(unsigned long long* out)
{
    for (int i = 0; i < 16; ++i) {
        out[i] = snappy_hip::g_alias_stats[i];
        snappy_hip::g_alias_stats[i] = 0;
    }
}
}
