"""Fine-level passes (levels 0-2) at a batch whose resident launch fits the chip: per-kernel hipEvent averages."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.util import pair
from pointcloudcounterfactual_amd import _lib, backend
if os.environ.get('PCC_AM_NORESIDENT') == '1':  # (tool-side switch; the library itself reads no behaviour variables)
    os.environ['PCC_TEST_HOOKS'] = '1'; _lib.set_tuning('am_noresident', 1)
dev = torch.device('cuda:0')
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
a, c = pair(1236, B, 2048, 2048)
t1, t2 = torch.from_numpy(a).to(dev), torch.from_numpy(c).to(dev)
for _ in range(5): backend.MatchCostImplicit(t1, t2, True)
torch.cuda.synchronize()
tot = 0.0
with _lib.profile() as read:
    for _ in range(10): backend.MatchCostImplicit(t1, t2, True)
    torch.cuda.synchronize()
    for name in ['am_fine_persist_kernel', 'am_phase_kernel<A> L0'] + ['am_phase_kernel<B> L%d' % i for i in range(3)] + ['am_phase_kernel<CA> L%d' % i for i in range(3)]:
        us, n = read(name)
        if n:
            print(f'  {name:28s} {us:7.1f} us x{n}'); tot += us
print(f'B={B} resident={os.environ.get("PCC_AM_NORESIDENT") != "1"}: fine levels total {tot:.1f} us')
