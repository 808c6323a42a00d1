"""Symbol rate of dvbs2_symsync_work_device for notes/symsync.md: 1, 64, 256 and 1024 streams, polyphase and linear at 2 samples per
symbol. Each figure is the median of five HIP-event regions after a warm-up call; the handle is reset before every region so that
each region walks the same samples. Prints one JSON line per point."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from dvbs2rx_amd import SymbolSync
    import symsync_model as S
    nsyms = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    x = S.qpsk_stream(seed=1, sps=2, nsyms=nsyms, rolloff=0.2, ppm=50.0, noise=0.1, matched=False)[0]
    st = torch.cuda.current_stream().cuda_stream
    for interp, name in ((0, "polyphase"), (1, "linear")):
        for ns in (1, 64, 256, 1024):
            ss = SymbolSync(sps=2, interp_method=interp, max_streams=ns, max_samples=x.size)
            d_in = torch.from_numpy(np.tile(x.view(np.float32), (ns, 1))).cuda()
            d_out = torch.zeros((ns, x.size), dtype=torch.float32, device="cuda")  # x.size / 2 symbols of two floats
            ms = []
            for region in range(6):
                ss.reset()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ss.work_device(d_in.data_ptr(), x.size, [x.size] * ns, d_out.data_ptr(), x.size // 2, x.size // 2, 0, 0, st)
                b.record()
                n_out, consumed, status = ss.finish()
                torch.cuda.synchronize()
                if region:
                    ms.append(a.elapsed_time(b))
            assert (status == 0).all()
            med = float(np.median(ms))
            print(json.dumps(dict(interp=name, streams=ns, symbols_per_stream=int(n_out[0]), regions_ms=[round(m, 3) for m in ms], median_ms=round(med, 3),
                                  msym_per_s_per_stream=round(int(n_out[0]) / med * 1e-3, 3), msym_per_s_total=round(int(n_out.sum()) / med * 1e-3, 2))))
            ss.close()


if __name__ == "__main__":
    main()
