"""The recall fixture (tests/golden/recall_vitl14.npz) through an fp32 torch forward of the sharpened ViT-L/14 with ONE tensor class
rounded to fp16 at a time: which class flips (query, k) outcomes of set_precision("fp16").  Classes: w_in (in_proj / c_fc weights),
w_out (out_proj / c_proj weights), qkv, P (attention probabilities), attn_out, hidden (MLP), patch (conv weight, patches, read-out row,
projection), stream (the residual stream stored in fp16, as the folded tower flow keeps it).  Prints flips, changed target ranks and
the gallery features' rel-L2 against the reference per set.  Run on the GPU box from the repository root:
    python tools/fp16_class_attribution.py
"""
import sys, os
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
from oracle import keds_oracle as O
from tests.conftest import golden_path

torch.backends.cuda.matmul.allow_tf32 = False
torch.set_float32_matmul_precision("highest")
VITL = dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14,
            context_length=77, vocab_size=49408, transformer_width=768, transformer_layers=12)
sd = {k: v.cuda().float() for k, v in O.sharpen_clip(O.synth_clip_state_dict(**VITL, seed=7)).items() if k.startswith("visual.")}
g = dict(np.load(golden_path("recall_vitl14.npz")))
G, Q = g["gallery"].shape[0], g["query"].shape[0]
tgt, ref, sigma = O.synth_recall_plan(G, Q)
imgs = [O.synth_gallery_images(min(125, G - i), start=i) for i in range(0, G, 125)]
qimgs = [O.synth_recall_queries(tgt, sigma, start=i, count=min(128, Q - i)) for i in range(0, Q, 128)]
H, W = 16, 1024


def fwd(img, cls):
    R = lambda t, c: t.half().float() if c in cls else t
    x = O.patch_embed({**sd, "visual.conv1.weight": R(sd["visual.conv1.weight"], "patch")}, R(img, "patch"))
    x = R(O.layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"]), "stream")
    B, S, _ = x.shape
    for i in range(24):
        p = f"visual.transformer.resblocks.{i}."
        h = O.layer_norm(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        qkv = R(O.linear(h, R(sd[p + "attn.in_proj_weight"], "w_in"), sd[p + "attn.in_proj_bias"]), "qkv")
        q, k, v = (t.reshape(B, S, H, 64).transpose(1, 2) for t in qkv.split(W, -1))
        P = R(torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1), "P")
        a = R((P @ v).transpose(1, 2).reshape(B, S, W), "attn_out")
        x = R(x + O.linear(a, R(sd[p + "attn.out_proj.weight"], "w_out"), sd[p + "attn.out_proj.bias"]), "stream")
        h = O.layer_norm(x, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        hid = R(O.quick_gelu(O.linear(h, R(sd[p + "mlp.c_fc.weight"], "w_in"), sd[p + "mlp.c_fc.bias"])), "hidden")
        x = R(x + O.linear(hid, R(sd[p + "mlp.c_proj.weight"], "w_out"), sd[p + "mlp.c_proj.bias"]), "stream")
    c = R(O.layer_norm(x[:, 0, :], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]), "patch")
    return torch.nn.functional.normalize(c @ R(sd["visual.proj"], "patch"), dim=-1)


KS = (1, 5, 10, 50, 100)
dr = 1.0 - torch.from_numpy(g["query"]) @ torch.from_numpy(g["gallery"]).T
rows, tg, rf = torch.arange(Q), torch.from_numpy(tgt), torch.from_numpy(ref)
dr[rows, rf] = float("inf")
rank_r = (dr < dr[rows, tg][:, None]).sum(1)
ALL = ("w_in", "w_out", "qkv", "P", "attn_out", "hidden", "patch", "stream")
for cls in [(), ("w_in",), ("w_out",), ("qkv",), ("P",), ("attn_out",), ("hidden",), ("patch",), ("stream",), ALL,
            tuple(c for c in ALL if c != "stream")]:
    with torch.no_grad():
        gal = torch.cat([fwd(im.cuda(), cls) for im in imgs]).cpu()
        qf = torch.cat([fwd(im.cuda(), cls) for im in qimgs]).cpu()
    dg = 1.0 - qf @ gal.T
    dg[rows, rf] = float("inf")
    rank_g = (dg < dg[rows, tg][:, None]).sum(1)
    flipped = sum(int(((rank_r < k) != (rank_g < k)).sum()) for k in KS)
    rel = float((gal - torch.from_numpy(g["gallery"])).norm() / torch.from_numpy(g["gallery"]).norm())
    print("fp16:", "+".join(cls) if cls else "(none)", "flipped", flipped, "target_rank_changes", int((rank_r != rank_g).sum()),
          "rel_l2_gallery", f"{rel:.3g}", flush=True)
