// query_columns_check.cpp — the column arithmetic of a host-pointer call (luisarender_amd/csrc/hip/query_columns.h) without a device, for the
// sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o query_columns_check tools/query_columns_check.cpp && ./query_columns_check
// For counts 0, 1, 2^20, 2^20 + 65 and 2^31 - 1 it walks the chunks of a call as staged_call does and checks that they partition the records
// in order, that only the last one is ragged, that every column's bytes of a chunk lie inside the caller's array and fit the column's slot,
// and that an absent column moves nothing.  Where the arrays are small enough to allocate (up to 2^20 + 65 records) it also plays the copies
// through host memory -- in, a stand-in launch, out -- so that AddressSanitizer sees every byte the routine would touch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../luisarender_amd/csrc/hip/query_columns.h"

using namespace lrh;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s (count %llu)\n", __FILE__, __LINE__, #cond, static_cast<unsigned long long>(g_count)); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

static uint64_t g_count = 0u;

// the spans of `columns` over every chunk of `count` records, against arrays that start at `columns[c].host`
static void check_spans(const std::vector<Column> &columns, uint64_t count) {
    g_count = count;
    CHECK(chunk_count(count) == (count + kQueryChunk - 1u) / kQueryChunk);
    CHECK((count == 0u) == (chunk_count(count) == 0u));
    uint64_t next = 0u;
    for (uint64_t i = 0u; i < chunk_count(count); i++) {
        const auto span = chunk_span(count, i);
        CHECK(span.first == next && span.n >= 1u && span.n <= kQueryChunk);
        CHECK(span.n == kQueryChunk || i + 1u == chunk_count(count));// only the last chunk is ragged
        next += span.n;
        for (auto &c : columns) {
            const auto s = column_span(c, span);
            if (c.host == nullptr) {
                CHECK(s.host == nullptr && s.bytes == 0u && slot_bytes(c, count) == 0u);
                continue;
            }
            CHECK(s.host == static_cast<char *>(c.host) + span.first * c.bytes);
            CHECK(s.bytes == span.n * c.bytes && s.bytes <= slot_bytes(c, count));
            CHECK(span.first * c.bytes + s.bytes <= count * c.bytes);// inside the caller's array
        }
    }
    CHECK(next == count);
    for (auto &c : columns) {
        if (c.host != nullptr) { CHECK(slot_bytes(c, count) == (count < kQueryChunk ? count : kQueryChunk) * c.bytes); }
    }
}

// a call played through host memory: out[k] = in[k] + 1 for every record, state[k] += 1, `cleared` written from zero
static void play(uint64_t count, bool with_optional) {
    g_count = count;
    std::vector<uint32_t> in(count), optional(with_optional ? count : 0u), out(count, 0xdeadbeefu), state(count), cleared(count * 4u, 0xdeadbeefu);
    for (uint64_t k = 0u; k < count; k++) { in[k] = static_cast<uint32_t>(k), state[k] = static_cast<uint32_t>(k * 3u); }
    for (uint64_t k = 0u; k < optional.size(); k++) { optional[k] = static_cast<uint32_t>(k * 7u); }
    const std::vector<Column> columns = {column_out(count != 0u ? out.data() : nullptr, sizeof(uint32_t)),
                                         column_in(count != 0u ? in.data() : nullptr, sizeof(uint32_t)),
                                         column_in(with_optional && count != 0u ? optional.data() : nullptr, sizeof(uint32_t)),
                                         Column{count != 0u ? state.data() : nullptr, sizeof(uint32_t), kColumnInOut},
                                         Column{count != 0u ? cleared.data() : nullptr, 4u * sizeof(uint32_t), kColumnClear}};
    check_spans(columns, count);
    std::vector<std::vector<char>> slots;// exactly as large as staged_call makes them: the sanitizer sees an overrun
    for (auto &c : columns) { slots.emplace_back(slot_bytes(c, count)); }
    for (uint64_t i = 0u; i < chunk_count(count); i++) {
        const auto span = chunk_span(count, i);
        for (size_t c = 0u; c < columns.size(); c++) {
            const auto s = column_span(columns[c], span);
            if (s.host == nullptr) { continue; }
            if ((columns[c].use & kColumnIn) != 0u) { std::memcpy(slots[c].data(), s.host, s.bytes); }
            if (columns[c].use == kColumnClear) { std::memset(slots[c].data(), 0, s.bytes); }
        }
        // the stand-in launch over records [first, first + n) of the slots
        const auto d_out = reinterpret_cast<uint32_t *>(slots[0].data());
        const auto d_in = reinterpret_cast<const uint32_t *>(slots[1].data());
        const auto d_optional = with_optional ? reinterpret_cast<const uint32_t *>(slots[2].data()) : nullptr;
        const auto d_state = reinterpret_cast<uint32_t *>(slots[3].data());
        const auto d_cleared = reinterpret_cast<uint32_t *>(slots[4].data());
        for (uint64_t k = 0u; k < span.n; k++) {
            d_out[k] = d_in[k] + 1u + (d_optional != nullptr ? d_optional[k] : 0u);
            d_state[k] += 1u;
            d_cleared[k * 4u + 3u] += static_cast<uint32_t>(span.first + k);
        }
        for (size_t c = 0u; c < columns.size(); c++) {
            const auto s = column_span(columns[c], span);
            if (s.host != nullptr && (columns[c].use & kColumnOut) != 0u) { std::memcpy(s.host, slots[c].data(), s.bytes); }
        }
    }
    for (uint64_t k = 0u; k < count; k++) {
        CHECK(out[k] == static_cast<uint32_t>(k) + 1u + (with_optional ? static_cast<uint32_t>(k * 7u) : 0u));
        CHECK(in[k] == static_cast<uint32_t>(k) && state[k] == static_cast<uint32_t>(k * 3u) + 1u);
        CHECK(cleared[k * 4u] == 0u && cleared[k * 4u + 3u] == static_cast<uint32_t>(k));
    }
}

int main() {
    // every count: the spans alone, against addresses that are never dereferenced (the widest column is the sampler's 512 bytes per record)
    const auto base = reinterpret_cast<char *>(uintptr_t{1} << 40u);
    for (uint64_t count : {uint64_t{0}, uint64_t{1}, kQueryChunk, kQueryChunk + 65u, (uint64_t{1} << 31u) - 1u}) {
        check_spans({column_out(base, 512u), column_in(base, 32u), column_in(nullptr, 32u), Column{base, 16u, kColumnInOut}, Column{base, 4u, kColumnClear}},
                    count);
    }
    // the counts whose arrays fit: the copies themselves
    for (uint64_t count : {uint64_t{0}, uint64_t{1}, kQueryChunk, kQueryChunk + 65u}) {
        play(count, true);
        play(count, false);
    }
    std::puts("query columns: ok");
    return 0;
}
