// The shared device pieces (pim-compression_amd/csrc/snappy_device_common.hpp) on the CPU wave emulator, each driven alone:
// a library of its own, built by tests/test_device_common_emulated.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_device_common.hpp"

extern "C" {

// workgroup_exclusive_scan in a 1024-thread workgroup that loops over `count` values as the planners do, its carry in a
// register: prefix[i] = sum of values[0..i), *total = sum of all
void emu_common_scan(const uint64_t* values, uint32_t count, uint64_t* prefix, uint64_t* total)
{
    emu::launch(1, 1024, [&] {
        __shared__ uint64_t wave_sums[16];
        const uint32_t tid = threadIdx.x;
        uint64_t carry = 0;
        for (uint32_t base = 0; base < count; base += 1024) {
            const uint32_t i = base + tid;
            uint64_t sum;
            const uint64_t at = carry + snappy_hip::workgroup_exclusive_scan(i < count ? values[i] : 0, wave_sums, sum);
            if (i < count) prefix[i] = at;
            carry += sum;
        }
        if (tid == 0) *total = carry;
    });
}

// workgroup_copy by one workgroup of 256 threads, wave_copy by one wavefront
void emu_common_workgroup_copy(uint8_t* dst, const uint8_t* src, uint32_t len)
{
    emu::launch(1, 256, [&] { snappy_hip::workgroup_copy(dst, src, len); });
}
void emu_common_wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len)
{
    emu::launch(1, 64, [&] { snappy_hip::wave_copy(dst, src, len, threadIdx.x); });
}

// owner[k] = prefix_owner<vector_loads>(prefix, count, p[k]), by one wavefront
void emu_common_prefix_owner(const uint64_t* prefix, uint32_t count, const uint32_t* p, uint32_t n, uint32_t* owner, int vector_loads)
{
    emu::launch(1, 64, [&] {
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t i = vector_loads ? snappy_hip::prefix_owner<true>(prefix, count, p[k]) : snappy_hip::prefix_owner<false>(prefix, count, p[k]);
            if (threadIdx.x == 0) owner[k] = i;
        }
    });
}

// put_varint32(out, v) -> its return value; *len = varint32_len(v).  out: 8 bytes.
uint32_t emu_common_varint(uint32_t v, uint8_t* out, uint32_t* len)
{
    uint32_t put = 0;
    emu::launch(1, 64, [&] {
        if (threadIdx.x == 0) {
            put = snappy_hip::put_varint32(out, v);
            *len = snappy_hip::varint32_len(v);
        }
    });
    return put;
}

}
