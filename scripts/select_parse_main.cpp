// A stand-alone host program over the selector parser of csrc/mn_select.hip, for sanitizer builds (scripts/check_select_parse.py):
// reads selectors, one per line in hexadecimal, and prints each one's postfix program or error message, in hexadecimal too.
#include "../include/muninn_hip.h"

#include <cstdarg>
#include <cstdio>
#include <iostream>
#include <string>

static std::string last_error;
void gset_err(const char *fmt, ...) { // mn_graph.hip's, which this program does not link
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error = buf;
}
extern "C" const char *mn_graph_last_error(void) { return last_error.c_str(); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::string text;
        for (size_t i = 0; i + 1 < line.size(); i += 2)
            text.push_back((char)std::stoi(line.substr(i, 2), nullptr, 16));
        mn_select_op *prog = nullptr;
        int n = 0;
        if (mn_select_parse(text.c_str(), &prog, &n) != 0) {
            printf("E");
            for (unsigned char c : last_error)
                printf("%02x", c);
            printf("\n");
            continue;
        }
        printf("P");
        for (int i = 0; i < n; i++) {
            printf(" %d:%d:%d:", prog[i].op, prog[i].depth_up, prog[i].depth_down);
            for (int k = 0; k < prog[i].name_len; k++)
                printf("%02x", (unsigned char)text[(size_t)(prog[i].name_off + k)]);
        }
        printf("\n");
        free(prog);
    }
    return 0;
}
