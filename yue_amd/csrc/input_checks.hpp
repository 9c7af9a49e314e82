// The checks of what a caller uploads as row lists -- ptr[rows + 1] and ids -- before a kernel indexes with them (DESIGN.md
// 5.000000).  Host code only: no HIP call, no kernel header, so that a stand-alone program can test it under the host's
// sanitizers (tests/helpers/input_checks_main.cpp).  Every refusal is YUE_ERR_ARG with a text that starts with `at`, the
// entry point and the list ("yue_knn_set_pairs: user-major"), and names the row where a row is at fault.
#pragma once
#include "../../include/yue_hip.h"

#include <algorithm>
#include <cstdint>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

namespace yue_host {

int fail(int code, const std::string &msg);          // sets the thread-local message of yue_last_error(), returns code

enum class Order { any, distinct, ascending };       // of the ids within a row: no rule / no id twice / strictly ascending
constexpr int64_t kNoTotal = -1;                     // the ABI passes no nnz: ptr[rows] is the length by contract
constexpr int64_t kNoLimit = std::numeric_limits<int64_t>::max();
struct NoRule { const char *operator()(int64_t, int64_t) const { return nullptr; } };

// One row list.  The WHOLE pointer first: not null, from 0, never down, no row longer than max_row, up to `total` when one is
// given; then ids not null when there are any; only then the ids, each in [0, bound) and in `order`.  So no ids[e] with
// e >= ptr[rows] is ever read, whatever the pointer holds.  rule(row, e) is what one subsystem alone asks of entry e (a
// count, a weight, no diagonal): the words of its fault, or nullptr.
template <class Rule = NoRule>
int check_rows(const std::string &at, const int64_t *ptr, int64_t rows, const int32_t *ids, int64_t bound, int64_t total, Order order,
               int64_t max_row = kNoLimit, Rule rule = Rule()) {
    if (!ptr) return fail(YUE_ERR_ARG, at + ": null pointer array");
    if (ptr[0] != 0) return fail(YUE_ERR_ARG, at + " pointer must start at 0");
    int64_t too_long = -1;                               // the first such row: said only when the pointer never falls
    for (int64_t r = 0; r < rows; ++r) {
        if (ptr[r + 1] < ptr[r]) return fail(YUE_ERR_ARG, at + " pointer must be non-decreasing (row " + std::to_string(r) + ")");
        if (ptr[r + 1] - ptr[r] > max_row && too_long < 0) too_long = r;
    }
    if (too_long >= 0) return fail(YUE_ERR_ARG, at + " row " + std::to_string(too_long) + " is too long (limit " + std::to_string(max_row) + ")");
    if (total != kNoTotal && ptr[rows] != total) return fail(YUE_ERR_ARG, at + " pointer must run from 0 to nnz");
    if (ptr[rows] > 0 && !ids) return fail(YUE_ERR_ARG, at + ": null id array");
    // the ids' range first, without a branch per id (FISM's rows lie in every call's time: 2 M ids of 100,000 rows take 0.5 ms
    // on a host core, the walk by rows 2 ms); the walk says which row, and is needed at all only for an order or a rule
    const uint32_t below = (uint32_t)std::min<int64_t>(std::max<int64_t>(bound, 0), (int64_t)1 << 31);      // (a negative id is a large one)
    const int64_t count = ptr[rows];
    unsigned bad = 0;
    for (int64_t e = 0; e < count; ++e) bad |= (unsigned)((uint32_t)ids[e] >= below);
    if (!bad && order == Order::any && std::is_same<Rule, NoRule>::value) return YUE_OK;
    std::vector<int64_t> mark(order == Order::distinct ? (size_t)bound : 0, -1);      // the last row that held an id
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t e = ptr[r]; e < ptr[r + 1]; ++e) {
            if (ids[e] < 0 || ids[e] >= bound) return fail(YUE_ERR_ARG, at + " id out of range (row " + std::to_string(r) + ")");
            if (order == Order::ascending && e > ptr[r] && ids[e] <= ids[e - 1]) return fail(YUE_ERR_ARG, at + " rows must be sorted and unique (row " + std::to_string(r) + ")");
            if (order == Order::distinct) {
                if (mark[(size_t)ids[e]] == r) return fail(YUE_ERR_ARG, at + " rows must hold distinct ids (row " + std::to_string(r) + ")");
                mark[(size_t)ids[e]] = r;
            }
            if (const char *words = rule(r, e)) return fail(YUE_ERR_ARG, at + " row " + std::to_string(r) + ": " + words);
        }
    return YUE_OK;
}

// The item-major pairs are the transpose of the user-major ones, for two lists that passed check_rows with Order::ascending
// and hold the same number of pairs: walking the users in order fills every item row in order, a cursor per item row.
// same(e, q) is what pair e of the user side and pair q of the item side must agree in beyond the ids (a count, a weight).
template <class Same>
int check_transpose(const std::string &at, int64_t m, const int64_t *u_ptr, const int32_t *u_items, int64_t n, const int64_t *i_ptr,
                    const int32_t *i_users, Same same) {
    std::vector<int64_t> cursor(i_ptr, i_ptr + n);
    for (int64_t u = 0; u < m; ++u)
        for (int64_t e = u_ptr[u]; e < u_ptr[u + 1]; ++e) {
            const int32_t i = u_items[e];
            const int64_t q = cursor[(size_t)i]++;
            if (q >= i_ptr[i + 1] || i_users[q] != (int32_t)u || !same(e, q))
                return fail(YUE_ERR_ARG, at + ": the item-major pairs are not the transpose of the user-major pairs (item " + std::to_string(i) + ")");
        }
    return YUE_OK;
}

// A plain array of ids, each in [0, bound).
inline int check_ids(const std::string &at, const int32_t *ids, int64_t count, int64_t bound) {
    for (int64_t t = 0; t < count; ++t)
        if (ids[t] < 0 || ids[t] >= bound) return fail(YUE_ERR_ARG, at + " id out of range (position " + std::to_string(t) + ")");
    return YUE_OK;
}

}  // namespace yue_host
