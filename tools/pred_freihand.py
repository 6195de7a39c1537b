"""FreiHAND evaluation-set prediction with a fine-tuned 2.5D hand-pose checkpoint (the reference's testing/pred_fh.py,
batched on the device):

    python tools/pred_freihand.py --model_path rn50_peclr_yt3d-fh_pt_fh_ft.pth --data /path/to/freihand [--batch 128]

Reads DIR/evaluation_K.json, DIR/evaluation_scale.json and DIR/evaluation/rgb/%08d.jpg (one image per K entry, 3960 in
the published set), infers the backbone from the file name ("rn50" / "rn152", as the reference does) and writes
out/pred_<type>.json and out/pred_<type>.zip in the working directory, ready for the evaluation server.

    python tools/pred_freihand.py --model_path ... --data /path/to/freihand --split training --eval

scores the model on a split that has labels instead: DIR/training_K.json, training_scale.json, training_xyz.json and the
first len(K) images of DIR/training/rgb/.  Every batch's prediction and ground truth go to a `PoseEvaluator` on the device;
the metric dict of the reference's evaluate() (Mean_EPE_3D, Median_EPE_3D, AUC and the three after Procrustes alignment) is
printed and written to out/eval_<type>.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--data", required=True, help="FreiHAND root (evaluation_K.json, evaluation_scale.json, evaluation/rgb/)")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--split", choices=("evaluation", "training"), default="evaluation")
    # (optional extras stay out of the namespace unless given: `vars(args)` of a plain call is what it always was)
    ap.add_argument("--precision", choices=("fp32", "bf16", "fp16"), default=argparse.SUPPRESS,
                    help="default fp32; bf16 / fp16: the backbone under autocast on the 16-bit kernels (crops, head and lifting stay fp32 / fp64)")
    ap.add_argument("--no-fold-bn", action="store_true", default=argparse.SUPPRESS,
                    help="16-bit: keep the BatchNorm passes (default: folded into the convolution epilogues)")
    ap.add_argument("--eval", action="store_true", help="score against DIR/<split>_xyz.json instead of writing a submission")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    split = args.split
    xyz_path = os.path.join(args.data, f"{split}_xyz.json")
    if args.eval and not os.path.exists(xyz_path):
        raise SystemExit(f"--eval needs ground-truth joints, but {xyz_path} does not exist"
                         + (" (FreiHAND's evaluation split has no labels: use --split training)" if split == "evaluation" else ""))

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
    with open(os.path.join(args.data, f"{split}_K.json")) as f:
        K_all = np.array(json.load(f), dtype=np.float64)
    with open(os.path.join(args.data, f"{split}_scale.json")) as f:
        scale_all = np.array(json.load(f), dtype=np.float64)
    if len(K_all) != len(scale_all):
        raise SystemExit(f"{len(K_all)} camera matrices but {len(scale_all)} scales")
    if args.eval:
        with open(xyz_path) as f:
            xyz_gt = np.array(json.load(f), dtype=np.float64)
        if xyz_gt.shape != (len(K_all), 21, 3):
            raise SystemExit(f"{xyz_path}: expected [{len(K_all)}, 21, 3] joints, got {list(xyz_gt.shape)}")

    model = RN25DwMLPref(model_type)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu")["state_dict"])
    model = model.eval().to("cuda").enable_hip()
    pred = FreiHANDPredictor(model, precision=getattr(args, "precision", "fp32"), fold_bn=False if getattr(args, "no_fold_bn", False) else None)
    if args.eval:
        from peclr_amd.pose_eval import PoseEvaluator

        scorer = PoseEvaluator(len(K_all), dtype=torch.float64, device=pred.device)

    t0 = time.time()
    out = []
    for lo in range(0, len(K_all), args.batch):
        hi = min(lo + args.batch, len(K_all))
        imgs = np.stack([np.asarray(Image.open(os.path.join(args.data, split, "rgb", "%08d.jpg" % i)).convert("RGB"))
                         for i in range(lo, hi)])
        xyz = pred.predict(imgs, K_all[lo:hi], scale_all[lo:hi])
        if args.eval:
            scorer.update(xyz, torch.from_numpy(xyz_gt[lo:hi]).to(pred.device))
            continue
        out.append(xyz.cpu().numpy())
    if args.eval:
        metrics = scorer.compute()
        path = os.path.join("out", f"eval_{model_type}.json")
        os.makedirs("out", exist_ok=True)
        with open(path, "w") as f:
            json.dump({k: (v.tolist() if isinstance(v, np.ndarray) else float(v)) for k, v in metrics.items()}, f, indent=1)
        for k, v in metrics.items():
            if not isinstance(v, np.ndarray):
                print(f"{k}: {float(v):.6g}")
        print(f"Scored {len(K_all)} samples of the {split} split, wrote {path} ({time.time() - t0:.1f} s)")
        return metrics
    xyz = np.concatenate(out)
    path = write_freihand_submission(os.path.join("out", f"pred_{model_type}"), xyz)
    print(f"Dumped {len(xyz)} joints and {len(xyz)} verts predictions to {path} ({time.time() - t0:.1f} s)")


if __name__ == "__main__":
    main()
