import sys, os, json
ROOT=os.environ.get("GRAFT_REPO_ROOT", os.getcwd()); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT,"tests"))
import torch
import emergent_multiagent_strategies_amd as fa
from test_gpu_policy import _policies, _obs
out={}
det = "det" in sys.argv[1:]     # FixedCategorical.mode instead of a sample (no Gumbel noise)
attn = "attn" in sys.argv[1:]   # the instantiation that exports the attention maps (fa_policy_kernel<.., true>), into fixed buffers
for G,A,E in ((3,3,4096),(5,5,4096)):
    pols, packed = _policies(fa, G, A, 1)
    eng = fa.BatchedFortAttack(E, G, A, 20); obs=_obs(E,G+A,E)
    kw = dict(deterministic=det, attn_out=eng.new_attn_out()) if attn else dict(deterministic=det)
    for _ in range(5): eng.policy_act(obs, packed[0], packed[1], **kw)
    torch.cuda.synchronize()
    best=1e9
    for rep in range(3):
        a,b=torch.cuda.Event(enable_timing=True),torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50): eng.policy_act(obs, packed[0], packed[1], **kw)
        b.record(); torch.cuda.synchronize(); best=min(best,a.elapsed_time(b)*20)
    out["%dv%d"%(G,A)]=round(best,2)
print(json.dumps({"deterministic": det, "attn": attn, "kernel": eng.policy_variant(export_attention=attn),
                  "lib": os.environ.get("FA_LIBRARY","product").split("/")[-1], **out}))
