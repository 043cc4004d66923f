"""DAVIS J / F counts of one 480x854 sequence (80 frames, 3 objects): `Engine.davis_counts` on the device against
`data.boundary_counts_host`.  Device time from events around the call (memset + 2 launches + the 11.5 KB count read-back),
wall time of the call, and one host run; the two results must be equal.   python tools/davis_measures_time.py [reps]"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, '.')
from eosvos_amd import data
from eosvos_amd.engine import Engine

N, H, W, K = 80, 480, 854, 3
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rng = np.random.default_rng(0)
yy, xx = np.ogrid[:H, :W]
def frame(shift):
    lab = np.zeros((H, W), np.uint8)
    for o, (cy, cx, ry, rx) in enumerate([(160, 200, 90, 120), (300, 500, 120, 80), (240, 700, 60, 100)], 1):
        lab[((yy - cy) / ry) ** 2 + ((xx - cx - shift) / rx) ** 2 <= 1] = o
    return lab
gt = np.stack([frame(2 * f) for f in range(N)])
pred = gt.copy()
pred[rng.random(pred.shape) < 0.001] = 0                  # speckle: boundaries all over the objects
pred = np.stack([np.roll(p, 3, axis=0) for p in pred])

eng = Engine('resnet50', 64, 96, max_batch=1, device='cuda:0')
p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
dev = eng.davis_counts(p, g, K)                            # warm-up (scratch allocation, code object load)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
dev_ms, wall_ms = [], []
for _ in range(REPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    dev = eng.davis_counts(p, g, K)
    ev1.record()
    ev1.synchronize()
    wall_ms.append(1e3 * (time.perf_counter() - t0))
    dev_ms.append(ev0.elapsed_time(ev1))
t0 = time.perf_counter()
host = data.boundary_counts_host(pred, gt, K)
host_s = time.perf_counter() - t0
assert np.array_equal(dev, host), 'device and host counts differ'
print(json.dumps({'frames': N, 'height': H, 'width': W, 'objects': K, 'radius': data.davis_bound_pix(0.008, H, W), 'reps': REPS,
                  'device_ms_median': round(float(np.median(dev_ms)), 4), 'device_ms_min': round(float(np.min(dev_ms)), 4),
                  'call_wall_ms_median': round(float(np.median(wall_ms)), 4), 'host_s': round(host_s, 3),
                  'boundary_pixels': int(host[..., 2:4].sum()), 'equal': True}))
eng.close()
