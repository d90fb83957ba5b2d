// query_columns.h — the column arithmetic of a host-pointer call (lrhip_query.hip: staged_call): which records are chunk i, and
// which bytes of which host column they are.  Plain C++ without a device, so that tools/query_columns_check.cpp can run it under the
// sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lrh {

// records per chunk of a host-pointer call: what a staging slot holds of a column, whatever the count (32 MiB of 32-byte records)
constexpr uint64_t kQueryChunk = 1ull << 20u;

// what a call does with a column
enum ColumnUse : uint32_t {
    kColumnIn = 1u,   // copied to the device before the launch
    kColumnOut = 2u,  // copied back after it
    kColumnInOut = 3u,// both: a sampler state, accumulated radiance
    kColumnClear = 6u,// cleared on the device instead of copied in, then copied back: radiance without LRHIP_RADIANCE_ACCUMULATE
};

// One array of a call, `bytes` per record.  host == nullptr: an optional column that is absent -- nothing is staged or copied, and the launch
// sees nullptr.  With LRHIP_RAY_DEVICE_POINTERS `host` is the caller's device pointer
struct Column {
    void *host;
    size_t bytes;
    uint32_t use;
};
inline Column column_in(const void *p, size_t bytes) { return {const_cast<void *>(p), bytes, kColumnIn}; }
inline Column column_out(void *p, size_t bytes) { return {p, bytes, kColumnOut}; }

struct ChunkSpan {
    uint64_t first, n;// records [first, first + n)
};
constexpr uint64_t chunk_count(uint64_t count) { return (count + kQueryChunk - 1u) / kQueryChunk; }
// chunk i < chunk_count(count): full chunks, then the ragged rest
constexpr ChunkSpan chunk_span(uint64_t count, uint64_t i) {
    return {i * kQueryChunk, count - i * kQueryChunk < kQueryChunk ? count - i * kQueryChunk : kQueryChunk};
}
// bytes a column's staging slot must hold for a call of `count` records (0: the column is absent or empty, no slot is touched)
constexpr size_t slot_bytes(const Column &c, uint64_t count) {
    return c.host == nullptr ? 0u : static_cast<size_t>(count < kQueryChunk ? count : kQueryChunk) * c.bytes;
}

struct ColumnSpan {
    char *host;  // where the chunk's records of the column start in the caller's array (nullptr: absent)
    size_t bytes;// how many bytes they are; they go to / come from the START of the column's slot
};
inline ColumnSpan column_span(const Column &c, ChunkSpan s) {
    if (c.host == nullptr) { return {nullptr, 0u}; }
    return {static_cast<char *>(c.host) + static_cast<size_t>(s.first) * c.bytes, static_cast<size_t>(s.n) * c.bytes};
}

}// namespace lrh
