// The option table (yue_amd/csrc/options_host.hip) on its own, for tests/test_option_table.py: a value-initialised context,
// no device and no subsystem.  Commands on stdin, fields separated by tabs (names may be empty or hold blanks):
//   g <name>            -> "<rc>\t<value>"    or "<rc>\t<message>"
//   s <name> <value>    -> "<rc>\t"           or "<rc>\t<message>"
// Built with the host's address and undefined-behaviour sanitizers and run directly.
#include "../../yue_amd/csrc/host_common.hpp"

#include <iostream>

static std::string g_message;

namespace yue_host {
int fail(int code, const std::string &msg) { g_message = msg; return code; }
bool fold_path(const yue_ctx *) { return true; }               // (what a context without factors answers)
int64_t wrmf_long_rows(const yue_ctx *, int) { return 0; }     // the subsystems' readers: no state
int64_t cof_levels(const yue_ctx *) { return 0; }
int64_t cof_cooccur_nnz(const yue_ctx *) { return 0; }
int64_t s2v_levels(const yue_ctx *, int) { return 0; }
}  // namespace yue_host

int main() {
    yue_ctx ctx{};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<std::string> f;
        for (size_t at = 0;;) {
            const size_t tab = line.find('\t', at);
            f.push_back(line.substr(at, tab == std::string::npos ? tab : tab - at));
            if (tab == std::string::npos) break;
            at = tab + 1;
        }
        int rc;
        int64_t value = 0;
        if (f.size() == 2 && f[0] == "g") {
            rc = yue_get_option(&ctx, f[1].c_str(), &value);
            std::cout << rc << '\t' << (rc == YUE_OK ? std::to_string(value) : g_message) << '\n';
        } else if (f.size() == 3 && f[0] == "s") {
            rc = yue_set_option(&ctx, f[1].c_str(), std::stoll(f[2]));
            std::cout << rc << '\t' << (rc == YUE_OK ? std::string() : g_message) << '\n';
        } else {
            std::cerr << "option_table_main: bad command: " << line << '\n';
            return 2;
        }
    }
    return 0;
}
