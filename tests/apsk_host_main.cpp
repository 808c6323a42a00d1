// apsk_host_main.cpp -- drives dvbs2rx_hip::xfecframe_demapper_cb (host/dvbs2rx_hip_blocks.h) on a 16APSK / 32APSK symbol file the way
// a GNU Radio scheduler would: forecast() + general_work() with a fixed SNR, then the llr_pdu refinement fed with the block's own LLRs.
// usage: apsk_host_main in.bin out.bin framesize rate_name constellation snr_lin
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../gr-dvbs2rx_amd/host/dvbs2rx_hip_blocks.h"
using namespace dvbs2rx_hip;

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> in;
    float buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    try {
        const int rate = dvbs2_rate_from_name(argv[4]);
        auto blk = xfecframe_demapper_cb::make((dvb_framesize_t)atoi(argv[3]), rate, (dvb_constellation_t)atoi(argv[5]), 4);
        gr_vector_int req(1), ninput(1);
        blk->forecast(blk->output_multiple(), req); // symbols per frame
        const int n_frames = (int)(in.size() / 2 / (size_t)req[0]);
        std::vector<int8_t> out((size_t)n_frames * blk->output_multiple());
        gr_vector_const_void_star ii(1, in.data());
        gr_vector_void_star oo(1, out.data());
        ninput[0] = n_frames * req[0];
        blk->set_snr_lin((float)atof(argv[6]));
        int consumed = 0;
        const int produced = blk->general_work((int)out.size(), ninput, ii, oo, &consumed);
        const int found = blk->handle_llr_pdu(0, n_frames, out.data(), out.size());
        f = fopen(argv[2], "wb");
        fwrite(out.data(), 1, (size_t)produced, f);
        fclose(f);
        printf("frames %d symbols_per_frame %d consumed %d produced %d found %d refined_snr_db %.4f\n", n_frames, req[0], consumed, produced, found, blk->get_snr());
        try {
            xfecframe_demapper_cb::make(FECFRAME_NORMAL, rate, MOD_8APSK);
            printf("8APSK accepted\n");
        } catch (const std::exception& e) { printf("8APSK: %s\n", e.what()); }
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
