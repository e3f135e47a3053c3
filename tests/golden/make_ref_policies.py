"""Writes tests/golden/ref_ppo_policies.npz: the 13 float32 tensors of two PPO policies the
reference ships as SB3 archives (policy_kwargs {}: SB3's default 64 x 64 Tanh MlpPolicy),

  hr       hr_sync_agent.zip                              O = 6, A = 1
  lorenz   code/lorenz_targeting_Lstm_continous_0.zip     O = 8, A = 3

Weights only: each archive's policy.pth is read with torch.load(weights_only=True), nothing
of the archive is executed, and the arrays are stored under "<name>/<SB3 key>".

  python tests/golden/make_ref_policies.py <reference checkout> [out.npz]
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
        "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
        "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
        "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
        "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "log_std")
ARCHIVES = {"hr": "hr_sync_agent.zip", "lorenz": "code/lorenz_targeting_Lstm_continous_0.zip"}


def main(ref_root, out):
    arrays = {}
    for name, rel in ARCHIVES.items():
        with zipfile.ZipFile(os.path.join(ref_root, rel)) as z:
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        for k in KEYS:
            a = sd[k].detach().numpy()
            assert a.dtype == np.float32, (name, k, a.dtype)
            arrays["%s/%s" % (name, k)] = np.ascontiguousarray(a)
        print(name, {k: tuple(sd[k].shape) for k in ("mlp_extractor.policy_net.0.weight", "action_net.weight")})
    np.savez(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "ref_ppo_policies.npz"))
