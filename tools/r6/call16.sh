#!/bin/bash
# GPU box, round 6 call 16: after the host-buffer change (dvbs2_host_alloc; no registration of numpy heap memory): the host tests, then the driver-style bench three times
O=gpurun_out/r6r; mkdir -p $O
timeout 900 python -m pytest tests/test_ldpc_gpu.py tests/test_shard_gloo.py tests/test_host_blocks.py -q -m gpu -k "host or page_locked or bench_n2 or rccl or copy" > $O/pytest.log 2>&1; echo "pytest rc $?"; tail -3 $O/pytest.log
for i in 1 2 3; do
  BENCH_TRACE=1 timeout 1200 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench$i.json 2> $O/bench$i.err; echo "bench $i rc $?"; grep -c "bench\]" $O/bench$i.err; grep -i "fault\|error" $O/bench$i.err | head -3
done
python - "$O" <<'PY'
import json, sys
for i in (1,2,3):
    try:
        d=json.loads([l for l in open(f"{sys.argv[1]}/bench{i}.json") if l.startswith('{')][-1])
    except Exception as e:
        print(i,'no json',e); continue
    c=d['configs']
    print(i,'headline',round(d['value']),'frac',round(d['roofline']['frac'],4),'c3',round(c['config3']['value']),'c4',round(c['config4']['value']),'c5',round(c['config5']['value']),'c5x',round(c['config5_s2x']['value']),
          'c2awgn',round(c['config2_awgn']['value']),c['config2_awgn']['frac_of_proportional_rate'],'c3awgn',round(c['config3_awgn']['value']),'c4awgn',round(c['config4_awgn']['value']),c['config4_awgn']['frac_of_proportional_rate'],
          'host',{k:round(v['frames_per_s']) for k,v in c['config2_host']['calls'].items()},'c3host',round(c['config3_host']['value']), c['config3_host']['operating_point']['calls'][f"4096_page_locked"]['frac_of_link_bound'], 'cpu', d.get('cpu_baseline',{}).get('value'))
PY
