// stdin rows "n_frames G page_locked symbols host_chunk host_plan" ("-": no plan) -> one line "first:frames first:frames ..." each
#include <cstdio>
#include <iostream>
#include "../gr-dvbs2rx_amd/csrc/host_plan.h"

int main()
{
    int n, G, locked, syms, hc;
    for (std::string hp; std::cin >> n >> G >> locked >> syms >> hc >> hp; std::printf("\n"))
        for (const auto& c : dvbs2::host_chunk_plan(n, G, locked, syms, hc, hp == "-" ? "" : hp)) std::printf("%d:%d ", c.first, c.second);
    return 0;
}
