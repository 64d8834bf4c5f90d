#!/usr/bin/env python3
"""One round of progressive distillation on MNIST (``train.DistillStep``): a conditional UNet that
samples in 2N DDIM steps teaches a copy of itself to sample in N - and, with ``--guidance-scale w``, a first rung of
guidance distillation before it (``train.GuidanceDistillStep``): a v-student learns the teacher's
classifier-free-guided output at every timestep, then teaches the round, so the N-step student's samples are guided
samples from one evaluation per step.

    python3 tools/distill_mnist.py --data <dir with train-images-idx3-ubyte and train-labels-idx1-ubyte>
                                   [--teacher teacher.pt] [--teacher-prediction eps|v] [--student-steps 4]
                                   [--guidance-scale 3.0] [--guidance-steps 2000]
                                   [--steps 2000] [--batch 256] [--lr 1e-4] [--out student.pt]

The raw IDX files are read from disk (nothing is downloaded; without them the script says so and stops).  Without
``--teacher`` the teacher has its initial weights: the round then only shows the mechanics.  The student is saved as a
``state_dict``; give it back as ``--teacher --teacher-prediction v --student-steps N/2`` for the next round, WITHOUT
``--guidance-scale``: the guidance is in its weights."""
import argparse
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_idx(path):
    import numpy as np

    with open(path, "rb") as f:
        zero, dtype, ndim = struct.unpack(">HBB", f.read(4))
        if zero != 0 or dtype != 0x08:
            raise ValueError(f"{path} is not an IDX file of unsigned bytes")
        shape = struct.unpack(">" + "I" * ndim, f.read(4 * ndim))
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=os.path.join(ROOT, "data", "MNIST", "raw"))
    ap.add_argument("--teacher", default=None)
    ap.add_argument("--teacher-prediction", default="eps", choices=("eps", "v"))
    ap.add_argument("--student-steps", type=int, default=4)
    ap.add_argument("--guidance-scale", type=float, default=None,
                    help="first rung: distil the teacher's classifier-free guidance at this scale into a v-student")
    ap.add_argument("--guidance-steps", type=int, default=2000, help="optimisation steps of that first rung")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    files = [os.path.join(a.data, n) for n in ("train-images-idx3-ubyte", "train-labels-idx1-ubyte")]
    if not all(os.path.exists(f) for f in files):
        sys.exit(f"no MNIST bytes under {a.data} (train-images-idx3-ubyte, train-labels-idx1-ubyte): nothing to do")

    import torch

    from tiny_diffusion_amd.conditional_diffusion import ForwardProcess, NoiseModel, ddim_sample
    from tiny_diffusion_amd.data import DeviceImageDataset
    from tiny_diffusion_amd.schedule import truncated_snr_weights
    from tiny_diffusion_amd.train import DistillStep, GuidanceDistillStep

    dev = torch.device("cuda", torch.cuda.current_device())
    data = DeviceImageDataset(torch.from_numpy(read_idx(files[0]).copy()), dev)
    labels = torch.from_numpy(read_idx(files[1]).astype("int64")).to(dev)
    fp = ForwardProcess()

    def train(step, steps, what):
        done = 0
        while done < steps:
            order = torch.randperm(len(data), device=dev)
            for i in range(0, len(data) - a.batch + 1, a.batch):
                idx = order[i:i + a.batch]
                loss = step.step(data.batch(idx), labels[idx])
                done += 1
                if done % 100 == 0 or done == steps:
                    print(f"{what} step {done}: weighted loss {loss.item():.5f}", flush=True)
                if done == steps:
                    break

    common = dict(prediction="v", clip_denoised=True, loss_weighting=truncated_snr_weights(fp, "v"), lr=a.lr,
                  philox_seed=1, timestep_seed=2, ema_decay=0.999, ema_warmup=True)
    teacher = NoiseModel().to(dev)
    if a.teacher:
        teacher.load_state_dict(torch.load(a.teacher, map_location=dev))
    teacher_prediction = a.teacher_prediction
    if a.guidance_scale is not None:
        # the first rung: one evaluation of the student for the teacher's guided pair; its average teaches the round
        guided = NoiseModel().to(dev).train()
        guided.load_state_dict(teacher.state_dict())
        rung = GuidanceDistillStep(guided, teacher, fp, a.guidance_scale, teacher_prediction=teacher_prediction, **common)
        train(rung, a.guidance_steps, f"guidance (w = {a.guidance_scale})")
        with rung.ema_weights():
            teacher.load_state_dict(guided.state_dict())
        teacher_prediction = "v"
        del rung, guided
    student = NoiseModel().to(dev).train()
    student.load_state_dict(teacher.state_dict())
    step = DistillStep(student, teacher, fp, a.student_steps, teacher_prediction=teacher_prediction, **common)
    train(step, a.steps, "distillation")
    with step.ema_weights():
        y = torch.arange(16, device=dev) % 10
        x = ddim_sample(student, fp, dev, 16, y, timesteps=step.timesteps, prediction="v", clip_denoised=True)
        print(f"{a.student_steps}-step samples of the averaged student: mean {x.mean().item():.4f}, "
              f"min {x.min().item():.3f}, max {x.max().item():.3f}")
        if a.out:
            torch.save(student.state_dict(), a.out)
            print(f"saved {a.out}")


if __name__ == "__main__":
    main()
