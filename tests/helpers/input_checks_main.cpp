// The row-list checks (yue_amd/csrc/input_checks.hpp) on their own, for tests/test_input_checks.py: no device, no library.
// Commands on stdin, fields separated by tabs; a list is numbers separated by commas, "-" is an empty list and "null" a null
// pointer; every list becomes a heap allocation of exactly its length, so that the address sanitizer sees a stray read:
//   rows <ptr> <rows> <ids> <bound> <total or -> <any|distinct|ascending> <max_row or -> <entry the rule refuses or ->
//   transpose <m> <u_ptr> <u_items> <n> <i_ptr> <i_users> <e:q the predicate refuses or ->
//   ids <ids> <bound>
// Each answers "<rc>\t<message>" (the message empty when rc is 0).  Built with the host's address and undefined-behaviour
// sanitizers and run directly.
#include "../../yue_amd/csrc/input_checks.hpp"

#include <iostream>
#include <memory>

static std::string g_message;

namespace yue_host {
int fail(int code, const std::string &msg) { g_message = msg; return code; }
}  // namespace yue_host

template <class T>
struct List {
    std::unique_ptr<T[]> p;
    int64_t n = 0;
    explicit List(const std::string &text) {
        if (text == "null") return;
        std::vector<T> v;
        if (text != "-")
            for (size_t at = 0;;) {
                const size_t comma = text.find(',', at);
                v.push_back((T)std::stoll(text.substr(at, comma == std::string::npos ? comma : comma - at)));
                if (comma == std::string::npos) break;
                at = comma + 1;
            }
        n = (int64_t)v.size();
        p.reset(new T[v.size()]);
        for (size_t t = 0; t < v.size(); ++t) p[t] = v[t];
    }
};

static int64_t number(const std::string &text, int64_t none) { return text == "-" ? none : std::stoll(text); }

int main() {
    using namespace yue_host;
    const std::string at = "entry: list";
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<std::string> f;
        for (size_t pos = 0;;) {
            const size_t tab = line.find('\t', pos);
            f.push_back(line.substr(pos, tab == std::string::npos ? tab : tab - pos));
            if (tab == std::string::npos) break;
            pos = tab + 1;
        }
        int rc;
        g_message.clear();
        if (f.size() == 9 && f[0] == "rows") {
            const List<int64_t> ptr(f[1]);
            const List<int32_t> ids(f[3]);
            const Order order = f[6] == "any" ? Order::any : f[6] == "distinct" ? Order::distinct : Order::ascending;
            const int64_t bad = number(f[8], -1);
            if (bad < 0)
                rc = check_rows(at, ptr.p.get(), std::stoll(f[2]), ids.p.get(), std::stoll(f[4]), number(f[5], kNoTotal), order, number(f[7], kNoLimit));
            else
                rc = check_rows(at, ptr.p.get(), std::stoll(f[2]), ids.p.get(), std::stoll(f[4]), number(f[5], kNoTotal), order, number(f[7], kNoLimit),
                                [bad](int64_t, int64_t e) { return e == bad ? "the rule's words" : nullptr; });
        } else if (f.size() == 8 && f[0] == "transpose") {
            const List<int64_t> u_ptr(f[2]), i_ptr(f[5]);
            const List<int32_t> u_items(f[3]), i_users(f[6]);
            int64_t be = -1, bq = -1;
            if (f[7] != "-") { be = std::stoll(f[7]); bq = std::stoll(f[7].substr(f[7].find(':') + 1)); }
            rc = check_transpose("entry", std::stoll(f[1]), u_ptr.p.get(), u_items.p.get(), std::stoll(f[4]), i_ptr.p.get(), i_users.p.get(),
                                 [be, bq](int64_t e, int64_t q) { return !(e == be && q == bq); });
        } else if (f.size() == 3 && f[0] == "ids") {
            const List<int32_t> ids(f[1]);
            rc = check_ids(at, ids.p.get(), ids.n, std::stoll(f[2]));
        } else {
            std::cerr << "input_checks_main: bad command: " << line << '\n';
            return 2;
        }
        std::cout << rc << '\t' << (rc == YUE_OK ? std::string() : g_message) << '\n';
    }
    return 0;
}
