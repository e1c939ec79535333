"""Generate tests/golden/eval.npz by IMPORTING the reference's evaluation code on the CPU (the pattern of make_golden.py).

    python tests/golden/make_eval_golden.py <the reference's src directory>          (or REFERENCE_SRC in the environment)

Only the small inputs and the numbers the reference computes are stored; none of its text travels.  Import recipe: namespace shells for the
packages whose __init__ pulls in ROS / the simulator, EMPTY shell modules for what is not installed (cv2, pytorch_msssim, torchmetrics, tqdm,
matplotlib when absent, ...: every attribute of a shell is a shell, calling one returns a shell), .cuda() -> identity, device='cuda' -> 'cpu'.
`Renderer` in eval_helpers' namespace is replaced by a stand-in that returns recorded tensors (the reference's two raster passes: depth +
silhouette first, colour second), and a fake wandb run records what report_progress logs.

What is pinned (src/mapper/splatam/utils/eval_helpers.py, slam_external.py):
  report_progress(mapping=True)   PSNR, "Depth RMSE", Depth L1                       (:211-264)
  eval, both branches             psnr.txt, rmse.txt, l1.txt as it writes them       (:409-608; mapping_iters = 0 and no new Gaussians: the
                                  silhouette branch; otherwise the plain branch)
  calc_ssim                       of the same three pairs, unmasked                  (slam_external.py:54-97)
  align, evaluate_ate             on a 12-pose trajectory: a known rigid offset plus noise   (:24-78)
NOT pinned: the MS-SSIM and LPIPS of eval (both packages are shells here; what eval writes to ssim.txt / lpips.txt is the shells' zero).
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, FRAMES, SIL_THRES = 40, 56, 3, 0.98


class CudaToCpu(TorchFunctionMode):
    def __torch_function__(self, f, t, a=(), k=None):
        k = dict(k or {})
        if str(k.get("device", "")).startswith("cuda"):
            k["device"] = "cpu"
        return f(*a, **k)


class Shell(types.ModuleType):
    """an empty stand-in: attributes, items and calls give shells; as a number it is zero"""

    def __init__(self, name="shell"):
        super().__init__(name)
        self.__path__ = []

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Shell(self.__name__ + "." + k)

    def __call__(self, *a, **k):
        return Shell(self.__name__ + "()")

    def __getitem__(self, i):
        return Shell(self.__name__ + "[]")

    def __iter__(self):
        return iter((Shell(), Shell()))

    def cpu(self):
        return self

    def numpy(self):
        return np.float32(0.0)

    def item(self):
        return 0.0


def shells(*names):
    for nm in names:
        try:
            importlib.import_module(nm)
        except Exception:
            parts = nm.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), Shell(".".join(parts[:i])))


class Recorded:
    """`Renderer(raster_settings=cam)(**rendervar)`: hands out the recorded tensors in call order"""
    queue = []

    def __init__(self, raster_settings=None):
        pass

    def __call__(self, **kw):
        return Recorded.queue.pop(0), None, None, None


class FakeRun:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(dict(d))


def frames_data():
    """three rendered / target pairs: a textured target, a render close to it, a depth with holes, a silhouette around the threshold"""
    g = torch.Generator().manual_seed(1234)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    im, depth_sil, gt_color, gt_depth = [], [], [], []
    for f in range(FRAMES):
        tex = torch.stack([0.5 + 0.4 * torch.sin(xs / 9 + c + f) * torch.cos(ys / 7 - c) for c in range(3)])
        gt = (tex + 0.1 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
        gt = torch.round(gt * 255) / 255                                   # what the dataset hands over: bytes / 255
        r = gt + 0.05 * torch.randn(3, H, W, generator=g)
        d = 1.5 + 0.5 * torch.sin(xs / 11 + f) + 0.3 * torch.rand(H, W, generator=g)
        d = torch.where(torch.rand(H, W, generator=g) < 0.1, torch.zeros(()), d)
        rd = 1.5 + 0.5 * torch.sin(xs / 11 + f) + 0.15 + 0.05 * torch.randn(H, W, generator=g)
        sil = 0.9 + 0.1 * torch.rand(H, W, generator=g)
        sil[::7, ::5] = SIL_THRES                                           # exactly on the threshold: the strict compare leaves these out
        im.append(r); depth_sil.append(torch.stack([rd, sil, rd * rd])); gt_color.append(gt); gt_depth.append(d[None])
    return torch.stack(im), torch.stack(depth_sil), torch.stack(gt_color), torch.stack(gt_depth)


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_SRC")
    if not src:
        sys.exit(__doc__)
    for name, p in [("mapper", src + "/mapper"), ("mapper.splatam", src + "/mapper/splatam"), ("mapper.splatam.utils", src + "/mapper/splatam/utils")]:
        m = types.ModuleType(name)
        m.__path__ = [p]
        sys.modules[name] = m
    shells("cv2", "tqdm", "matplotlib", "matplotlib.pyplot", "pytorch_msssim", "torchmetrics", "torchmetrics.image", "torchmetrics.image.lpip",
           "kornia", "kornia.geometry", "kornia.geometry.linalg", "open3d", "wandb", "diff_gaussian_rasterization")
    torch.Tensor.cuda = lambda self, *a, **k: self
    with CudaToCpu():
        eh = importlib.import_module("mapper.splatam.utils.eval_helpers")
        from mapper.splatam.utils import recon_helpers, slam_external
        eh.Renderer = Recorded
        eh.tqdm = lambda it, *a, **k: it
        im, depth_sil, gt_color, gt_depth = frames_data()
        K = np.array([[W / 2.0, 0, W / 2.0 - 1, 0], [0, W / 2.0, H / 2.0 - 1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        params = dict(means3D=torch.rand(5, 3) + torch.tensor([0.0, 0.0, 2.0]), rgb_colors=torch.rand(5, 3), unnorm_rotations=torch.randn(5, 4),
                      logit_opacities=torch.zeros(5, 1), log_scales=torch.full((5, 1), -3.0),
                      cam_unnorm_rots=torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1).repeat(1, 1, FRAMES).contiguous(),
                      cam_trans=torch.zeros(1, 3, FRAMES))
        cam = recon_helpers.setup_camera(W, H, K[:3, :3], np.eye(4))
        out = dict(im=im.numpy(), depth_sil=depth_sil.numpy(), gt_color=gt_color.numpy(), gt_depth=gt_depth.numpy(), sil_thres=np.float64(SIL_THRES))

        # ---- report_progress(mapping=True): what it logs ----
        rp = []
        for f in range(FRAMES):
            run = FakeRun()
            Recorded.queue = [depth_sil[f], im[f]]
            data = {"cam": cam, "im": gt_color[f], "depth": gt_depth[f], "id": f, "intrinsics": torch.from_numpy(K[:3, :3]), "w2c": torch.eye(4)}
            eh.report_progress(params, data, 1, Shell("bar"), f, sil_thres=SIL_THRES, mapping=True, online_time_idx=f, wandb_run=run, wandb_step=0)
            log = run.logged[-1]
            rp.append([float(log["Mapping/PSNR"]), float(log["Mapping/Depth RMSE"]), float(log["Mapping/Depth L1"])])
        out["report_progress"] = np.array(rp, dtype=np.float64)

        # ---- eval, both branches: the text files it writes ----
        class Dataset:
            def __getitem__(self, t):
                color = torch.round(gt_color[t].permute(1, 2, 0) * 255)          # (the bytes: eval's / 255 gives gt_color back to the bit)
                return color, gt_depth[t].permute(1, 2, 0), torch.from_numpy(K), torch.eye(4)
        for key, iters, add in (("eval_sil", 0, False), ("eval_plain", 2, True)):
            Recorded.queue = [t for f in range(FRAMES) for t in (depth_sil[f], im[f])]
            with tempfile.TemporaryDirectory() as d:
                eh.eval(Dataset(), params, FRAMES, d, SIL_THRES, iters, add, wandb_run=FakeRun(), wandb_save_qual=False, eval_every=1)
                out[key] = np.stack([np.loadtxt(os.path.join(d, nm)).reshape(-1) for nm in ("psnr.txt", "rmse.txt", "l1.txt")], 1)
            assert out[key].shape == (FRAMES, 3) and not Recorded.queue

        # ---- calc_ssim of the same pairs ----
        out["calc_ssim"] = np.array([float(slam_external.calc_ssim(im[f], gt_color[f])) for f in range(FRAMES)], dtype=np.float64)

        # ---- align / evaluate_ate: 12 poses, a known rigid offset plus noise ----
        rng = np.random.default_rng(7)
        n = 12
        a = np.linspace(0, 2.5, n)
        pts = np.stack([np.cos(a) * 2, 0.1 * a, np.sin(a) * 2], 0) + 0.05 * rng.normal(size=(3, n))
        ang = 0.4
        Rm = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ \
            np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
        tv = np.array([[0.3], [-0.2], [0.5]])
        est = Rm @ pts + tv + 0.01 * rng.normal(size=(3, n))
        gt_list, est_list = [], []
        for i in range(n):
            g4, e4 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
            g4[:3, 3], e4[:3, 3] = pts[:, i], est[:, i]
            gt_list.append(torch.from_numpy(g4)); est_list.append(torch.from_numpy(e4))
        gp = torch.stack([m[:3, 3] for m in gt_list]).numpy().T
        ep = torch.stack([m[:3, 3] for m in est_list]).numpy().T
        rot, trans, err = eh.align(gp.astype(np.float64), ep.astype(np.float64))      # (the float32 values in fp64; evaluate_ate itself aligns in float32)
        out.update(ate_gt=torch.stack(gt_list).numpy(), ate_est=torch.stack(est_list).numpy(), ate=np.float64(eh.evaluate_ate(gt_list, est_list)),
                   align_rot=np.asarray(rot, dtype=np.float64), align_trans=np.asarray(trans, dtype=np.float64).reshape(3, 1),
                   align_error=np.asarray(err, dtype=np.float64).reshape(-1))
    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})
    print("report_progress", out["report_progress"], "\neval_sil", out["eval_sil"], "\neval_plain", out["eval_plain"], "\ncalc_ssim", out["calc_ssim"],
          "\nate", out["ate"])


if __name__ == "__main__":
    main()
