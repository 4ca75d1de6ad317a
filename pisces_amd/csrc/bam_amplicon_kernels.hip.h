// bam_amplicon_kernels.hip.h — the BAM XN tag (Read.GetAmpliconNameIfExists, Read.cs:483-486) of a decoded batch turned into one amplicon
// id per read without the records leaving the device.  bam_decode_kernel leaves, per kept read, where its name lies in the inflated
// stream (amp_tag: offset << 16 | length, kAmpNoTag without the tag); here the names are interned:
//   amplicon_intern_kernel      one lane per kept read: an open-addressing table in HBM, indexed by a hash of the name's bytes.  A slot is
//                               claimed with one 64-bit atomicCAS that writes the claimant's amp_tag word: that read is the slot's
//                               representative.  A lane that finds a slot taken compares its name with the representative's BYTES in the
//                               stream and stays only when they are equal (the hash decides where to look, never what is equal).  Every
//                               slot keeps the lowest read index that reached it, every read its slot.
//   amplicon_compact_kernel     one lane per slot: the occupied ones as (slot, first read, length, byte offset) with their bytes gathered
//                               into one buffer: all that goes to the host, as many entries as the batch has distinct names.
//   amplicon_assign_ids_kernel  the host's slot -> id table (the handle's dictionary, surface_bam.inc.h) applied: amp_ids[r], -1 without a tag.
// Which read represents a name and which slot the name lands in depend on the order the lanes arrive in; (name -> lowest read index)
// does not, and the ids are made from that alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pisces {

constexpr int kAmpTableSlots = 4096;                     // the table's first size (a power of two); four times larger while more than half is taken
constexpr unsigned long long kAmpNoTag = ~0ull;          // amp_tag of a read without the tag; an empty slot of the table
constexpr int32_t kAmpNoRead = 0x7FFFFFFF;               // a slot's first read before any read reached it

struct AmpliconName { int32_t slot, first_read, length, byte_offset; };

__device__ __forceinline__ unsigned long long amp_tag_of(int64_t offset, int length)   // (a stream holds less than 2^39 bytes, a record less than 2^15)
{
    return ((unsigned long long)offset << 16) | (unsigned long long)(uint32_t)length;
}

__device__ __forceinline__ bool amp_same_name(const uint8_t* __restrict__ s, unsigned long long a, unsigned long long b)
{
    if (a == b) return true;                             // the representative itself
    const uint32_t len = (uint32_t)(a & 0xFFFFull);
    if (len != (uint32_t)(b & 0xFFFFull)) return false;
    const uint8_t* const p = s + (a >> 16);
    const uint8_t* const q = s + (b >> 16);
    for (uint32_t k = 0; k < len; k++)
        if (p[k] != q[k]) return false;
    return true;
}

// words[0]: slots taken, words[1]: bytes of the representatives' names, words[2]: 1 when a read found no slot (a table that small is
// rerun larger: more than half of it is taken then)
__global__ __launch_bounds__(256) void amplicon_intern_kernel(const uint8_t* __restrict__ s, const unsigned long long* __restrict__ amp_tag, int32_t n_reads,
                                                              unsigned long long* __restrict__ table, int32_t* __restrict__ slot_first, uint32_t mask,
                                                              int32_t* __restrict__ read_slot, unsigned long long* __restrict__ words)
{
    const int32_t r = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (r >= n_reads) return;
    const unsigned long long tag = amp_tag[r];
    if (tag == kAmpNoTag) { read_slot[r] = -1; return; }
    const uint32_t len = (uint32_t)(tag & 0xFFFFull);
    const uint8_t* const name = s + (tag >> 16);
    uint32_t hash = 2166136261u;                         // FNV-1a, then a finishing mix: names that differ in their last byte leave neighbours otherwise
    for (uint32_t k = 0; k < len; k++) hash = (hash ^ name[k]) * 16777619u;
    hash ^= hash >> 15; hash *= 0x2C1B3C6Du; hash ^= hash >> 12;
    uint32_t i = hash & mask;
    for (uint32_t probes = 0; probes <= mask; probes++, i = (i + 1) & mask) {
        // load and test before each atomic: neighbouring reads share names, and a slot, once taken, never changes
        unsigned long long cur = __hip_atomic_load(table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kAmpNoTag) {
            cur = atomicCAS(table + i, kAmpNoTag, tag);
            if (cur == kAmpNoTag) {
                cur = tag;
                atomicAdd(words + 0, 1ull);
                atomicAdd(words + 1, (unsigned long long)len);
            }
        }
        if (!amp_same_name(s, tag, cur)) continue;
        if (__hip_atomic_load(slot_first + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > r) atomicMin(slot_first + i, r);
        read_slot[r] = (int32_t)i;
        return;
    }
    read_slot[r] = -1;
    words[2] = 1ull;
}

// counters[0]: entries written, counters[1]: name bytes written (both preset 0; the capacities are what the intern kernel counted)
__global__ __launch_bounds__(256) void amplicon_compact_kernel(const uint8_t* __restrict__ s, const unsigned long long* __restrict__ table,
                                                               const int32_t* __restrict__ slot_first, uint32_t n_slots, AmpliconName* __restrict__ names,
                                                               uint32_t name_capacity, uint8_t* __restrict__ bytes, uint32_t byte_capacity,
                                                               uint32_t* __restrict__ counters)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_slots) return;
    const unsigned long long tag = table[i];
    if (tag == kAmpNoTag) return;
    const uint32_t len = (uint32_t)(tag & 0xFFFFull);
    const uint32_t k = atomicAdd(counters + 0, 1u), at = atomicAdd(counters + 1, len);
    if (k >= name_capacity || at + len > byte_capacity) return;
    names[k] = {(int32_t)i, slot_first[i], (int32_t)len, (int32_t)at};
    const uint8_t* const name = s + (tag >> 16);
    for (uint32_t b = 0; b < len; b++) bytes[at + b] = name[b];
}

__global__ __launch_bounds__(256) void amplicon_assign_ids_kernel(const int32_t* __restrict__ read_slot, const int32_t* __restrict__ slot_id, int32_t n_reads,
                                                                  int32_t* __restrict__ amp_ids)
{
    const int32_t r = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (r >= n_reads) return;
    const int32_t slot = read_slot[r];
    amp_ids[r] = slot >= 0 ? slot_id[slot] : -1;
}

}  // namespace pisces
