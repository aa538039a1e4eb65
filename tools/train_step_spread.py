"""How far two training steps of ONE configuration differ in their gradients, with and without the sentinel-filled allocator of
tests/buffer_contract.py: cfg1, three views, the loss of tests/test_gpu_modules.py::test_three_sgd_steps_with_the_batched_weight_planes,
a fresh detector from one seed per step.  Per parameter: max |g_a - g_b| / max |g_plain| for two plain steps, a step under each sentinel
against a plain one, and the two sentinels against each other; and the same for two backward passes of ONE forward.  The bound of
tests/test_gpu_buffers.py::test_one_training_step_reads_no_capacity_tail comes from these figures (profiles/r20_train_step_spread.json).

    python tools/train_step_spread.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import sgcdet_amd.plugin  # noqa: E402,F401
from buffer_contract import prefilled  # noqa: E402
from sgcdet_amd import functions  # noqa: E402
from sgcdet_amd.mmcv_lite import build_detector  # noqa: E402
from sgcdet_amd.scene import make_scene, model_config, workload  # noqa: E402


def main(out):
    w = workload("cfg1_plumbing")
    feats, dpt, meta = make_scene(3, w["embed_dims"], kind="scannet", seed=14, device="cuda")
    planes = functions.train_weight_planes()

    def forward():
        torch.manual_seed(23)
        det = build_detector(model_config(w)).cuda().train()
        det.use_graph = det.scene_graph = False
        for m in det.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        planes.clear()
        r = det.forward_features(feats, [meta], dpt)
        loss = sum((t ** 2).mean() for k in ("centerness", "bbox_pred", "cls_score") for t in r[k]) + r["occ"].mean()
        return loss, [(k, p) for k, p in det.named_parameters() if p.requires_grad]

    def backward(loss, params):
        gs = torch.autograd.grad(loss, [p for _, p in params], retain_graph=True, allow_unused=True)
        torch.cuda.synchronize()
        return {k: g.detach().clone() for (k, _), g in zip(params, gs) if g is not None}

    def step(kind=None):
        if kind is None:
            loss, params = forward()
            return float(loss.detach()), backward(loss, params)
        with prefilled(kind):
            loss, params = forward()
            return float(loss.detach()), backward(loss, params)
    runs = {"plain1": step(), "plain2": step(), "plain3": step(), "A": step("A"), "B": step("B")}
    loss, params = forward()
    same = {"backward1": backward(loss, params), "backward2": backward(loss, params)}
    planes.clear()
    scale = {k: float(g.abs().max()) or 1.0 for k, g in runs["plain1"][1].items()}

    def rel(ga, gb):
        return {k: float((ga[k].double() - gb[k].double()).abs().max()) / scale[k] for k in scale}
    pairs = {"plain1_plain2": rel(runs["plain1"][1], runs["plain2"][1]), "plain1_plain3": rel(runs["plain1"][1], runs["plain3"][1]),
             "plain2_plain3": rel(runs["plain2"][1], runs["plain3"][1]), "plain1_A": rel(runs["plain1"][1], runs["A"][1]),
             "plain1_B": rel(runs["plain1"][1], runs["B"][1]), "A_B": rel(runs["A"][1], runs["B"][1]),
             "one_forward_two_backwards": rel(same["backward1"], same["backward2"])}
    worst = {name: dict(sorted(d.items(), key=lambda kv: -kv[1])[:8]) for name, d in pairs.items()}
    result = dict(what="max |g_a - g_b| / max |g_plain1| per parameter: the eight largest of every pair, and the largest of all",
                  losses={k: v[0] for k, v in runs.items()}, largest={name: max(d.values()) for name, d in pairs.items()},
                  max_abs_gradient={k: scale[k] for d in worst.values() for k in d}, worst=worst)
    print(json.dumps(dict(losses=result["losses"], largest=result["largest"]), indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
