// tree_plan_san.cpp -- TEST-ONLY stand-alone program (no Python): the tree build and trace planning of csrc/psdr_tree_plan.h through the one entry of
// hostcheck_plan.cpp (hostcheck_tree), meant to be compiled with -fsanitize=address,undefined (tests/test_tree_plan_host.py builds and runs it as a child
// process, over the cases it has just checked in the library).  No HIP call is made and no device is opened.
//   file   = one case per line: the rule's name, then its numbers
//   stdout = one line per case: the count hostcheck_tree returned, then the numbers it wrote
#include "hostcheck_plan.cpp"

#include <cstdio>
#include <sstream>

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: tree_plan_san <cases file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "tree_plan_san: cannot open %s\n", argv[1]); return 2; }
    std::string text;
    char buf[4096];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
    std::fclose(f);
    std::istringstream lines(text);
    for (std::string line; std::getline(lines, line);) {
        std::istringstream words(line);
        std::string what;
        if (!(words >> what)) continue;
        std::vector<double> in;
        for (std::string v; words >> v;) in.push_back(std::strtod(v.c_str(), nullptr));          // (strtod reads the hexadecimal floats Python's float.hex writes)
        std::vector<double> out(in.size() * 4 + 256);          // exactly what the front end passes as well
        const int m = hostcheck_tree(what.c_str(), in.data(), (int) in.size(), out.data());
        std::printf("%d", m);
        for (int i = 0; i < m; ++i) std::printf(" %a", out[(size_t) i]);
        std::printf("\n");
    }
    return 0;
}
