"""FreiHAND evaluation-set prediction with a fine-tuned 2.5D hand-pose checkpoint (the reference's testing/pred_fh.py,
batched on the device):

    python tools/pred_freihand.py --model_path rn50_peclr_yt3d-fh_pt_fh_ft.pth --data /path/to/freihand [--batch 128]

Reads DIR/evaluation_K.json, DIR/evaluation_scale.json and DIR/evaluation/rgb/%08d.jpg (one image per K entry, 3960 in
the published set), infers the backbone from the file name ("rn50" / "rn152", as the reference does) and writes
out/pred_<type>.json and out/pred_<type>.zip in the working directory, ready for the evaluation server.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--data", required=True, help="FreiHAND root (evaluation_K.json, evaluation_scale.json, evaluation/rgb/)")
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args(argv)

    import torch
    from PIL import Image

    from peclr_amd.pose import FreiHANDPredictor, RN25DwMLPref, write_freihand_submission

    name = os.path.basename(args.model_path)
    if "rn50" in name:
        model_type = "rn50"
    elif "rn152" in name:
        model_type = "rn152"
    else:
        raise SystemExit("Cannot infer model_type from model_path. Did you rename the .pth file?")
    with open(os.path.join(args.data, "evaluation_K.json")) as f:
        K_all = np.array(json.load(f), dtype=np.float64)
    with open(os.path.join(args.data, "evaluation_scale.json")) as f:
        scale_all = np.array(json.load(f), dtype=np.float64)
    if len(K_all) != len(scale_all):
        raise SystemExit(f"{len(K_all)} camera matrices but {len(scale_all)} scales")

    model = RN25DwMLPref(model_type)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu")["state_dict"])
    model = model.eval().to("cuda").enable_hip()
    pred = FreiHANDPredictor(model)

    t0 = time.time()
    out = []
    for lo in range(0, len(K_all), args.batch):
        hi = min(lo + args.batch, len(K_all))
        imgs = np.stack([np.asarray(Image.open(os.path.join(args.data, "evaluation", "rgb", "%08d.jpg" % i)).convert("RGB"))
                         for i in range(lo, hi)])
        out.append(pred.predict(imgs, K_all[lo:hi], scale_all[lo:hi]).cpu().numpy())
    xyz = np.concatenate(out)
    path = write_freihand_submission(os.path.join("out", f"pred_{model_type}"), xyz)
    print(f"Dumped {len(xyz)} joints and {len(xyz)} verts predictions to {path} ({time.time() - t0:.1f} s)")


if __name__ == "__main__":
    main()
