"""A student DAU network learns to reproduce a fixed teacher DAU layer: the drop-in Python surface (DAUConv2d with the
reference's constructor arguments) inside an ordinary PyTorch training loop.  Offsets (mu1, mu2) are learned through the
operator's own gradients; `mu_learning_rate_factor` scales them inside the op as in the reference
(plugins/tensorflow/src/dau_conv_grad_op.cpp:297-303).

    python examples/train_toy.py [--steps 60] [--compile [--backend inductor]] [--graph] [--conv1d]

--compile wraps the student in torch.compile: each DAU layer becomes one opaque op (torch.ops.dau_conv.conv) of a single graph, runs
the same kernels on the same bits, and the losses printed are those of the eager run.
--graph captures the whole training step -- zero_grad(set_to_none=True), forward, loss, backward and the optimizer step -- into one
graph (torch.cuda.graph) after three ordinary warm-up steps and replays it for the rest: no Python and no launch overhead per step, the
same kernels.  Adam runs with capturable=True there (its step count and bias correction on the device, in float32), so the losses
follow the eager run's closely but are not promised to be its digits.  The student's offsets and sigma may move in a replay; at the end
dau_conv.check_pending_offsets() is asked, as a replaying caller must ("Graph capture").
--conv1d trains a stack of single-dimension layers (DAUConv1d: offsets along x only) twice from the same seed, without and with
dense_line=True (calls whose units lie on a line run the 1 x 9 two-limb GEMM), and prints the two loss curves side by side.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dau-convnet_amd"))

import torch
import dau_conv


def run(steps=60, seed=0, verbose=True, compile=False, backend="inductor", graph=False):
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    teacher = dau_conv.DAUConv2d(filters=16, dau_units=(2, 2), max_kernel_size=9, use_bias=False, in_channels=8,
                                 mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                 mu2_initializer=dau_conv.random_uniform_initializer(-3, 3)).to(dev)
    for p in teacher.parameters():
        p.requires_grad_(False)
    student = torch.nn.Sequential(
        dau_conv.DAUConv2d(filters=16, dau_units=(2, 2), max_kernel_size=9, in_channels=8, activation=torch.relu,
                           mu_learning_rate_factor=10, fused_epilogue=True),      # bias and ReLU inside the kernels' store
        dau_conv.DAUConv2d(filters=16, dau_units=(2, 2), max_kernel_size=9, in_channels=16, use_bias=False,
                           mu_learning_rate_factor=10, fused_epilogue=True),
    ).to(dev)
    # (capturable: Adam keeps its step count on the device, which a captured step needs)
    opt = torch.optim.Adam(student.parameters(), lr=3e-3, capturable=bool(graph))
    model = torch.compile(student, backend=backend) if compile else student
    losses = []
    static_x = torch.empty(16, 8, 32, 32, device=dev)

    def train_step():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(model(static_x), teacher(static_x))
        loss.backward()
        opt.step()
        return loss

    warmup, captured, static_loss = 3, None, None
    side = torch.cuda.Stream()
    for step in range(steps):
        static_x.copy_(torch.rand(16, 8, 32, 32, device=dev))
        if not graph:
            loss = train_step()
        elif step < warmup:
            # ordinary steps on the stream the capture will use: every plan makes its first call, the optimizer builds its state
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                loss = train_step()
            torch.cuda.current_stream().wait_stream(side)
        else:
            if captured is None:
                torch.cuda.synchronize()
                captured = torch.cuda.CUDAGraph()
                with torch.cuda.graph(captured, stream=side):
                    static_loss = train_step()
            captured.replay()
            loss = static_loss
        losses.append(float(loss.detach()))
        if verbose and step % 10 == 0:
            print("step %3d  loss %.5f" % (step, losses[-1]))
    if graph:
        dau_conv.check_pending_offsets()         # offsets and sigma of the replays: a replay runs no Python that could raise
    return losses


def run_conv1d(steps=60, seed=0, dense_line=False, verbose=False):
    """The same task on DAUConv1d layers; dense_line: the line members of the two-limb gather-sum for the student's layers."""
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    teacher = dau_conv.DAUConv1d(filters=16, dau_units=(2, 1), max_kernel_size=9, use_bias=False, in_channels=8,
                                 mu1_initializer=dau_conv.random_uniform_initializer(-3, 3)).to(dev)
    for p in teacher.parameters():
        p.requires_grad_(False)
    student = torch.nn.Sequential(
        dau_conv.DAUConv1d(filters=16, dau_units=(2, 1), max_kernel_size=9, in_channels=8, activation=torch.relu,
                           mu_learning_rate_factor=10, fused_epilogue=True, dense_line=dense_line),
        dau_conv.DAUConv1d(filters=16, dau_units=(2, 1), max_kernel_size=9, in_channels=16, use_bias=False,
                           mu_learning_rate_factor=10, fused_epilogue=True, dense_line=dense_line),
    ).to(dev)
    opt = torch.optim.Adam(student.parameters(), lr=3e-3)
    losses = []
    for step in range(steps):
        x = torch.rand(16, 8, 32, 32, device=dev)
        loss = torch.nn.functional.mse_loss(student(x), teacher(x))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if verbose and step % 10 == 0:
            print("step %3d  loss %.5f" % (step, losses[-1]))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--compile", action="store_true", help="wrap the student in torch.compile")
    ap.add_argument("--backend", default="inductor", help="torch.compile backend (aot_eager needs no code generation)")
    ap.add_argument("--graph", action="store_true", help="capture the whole training step into one graph and replay it")
    ap.add_argument("--conv1d", action="store_true", help="DAUConv1d layers, without and with dense_line=True")
    args = ap.parse_args()
    if args.conv1d:
        off, on = run_conv1d(args.steps, dense_line=False), run_conv1d(args.steps, dense_line=True)
        print("step   loss            loss (dense_line=True)")
        for step in range(0, args.steps, 10):
            print("%4d   %.5f         %.5f" % (step, off[step], on[step]))
        print("loss %.5f -> %.5f   (dense_line=True: %.5f -> %.5f)" % (off[0], off[-1], on[0], on[-1]))
        sys.exit(0)
    l = run(args.steps, compile=args.compile, backend=args.backend, graph=args.graph)
    print("loss %.5f -> %.5f" % (l[0], l[-1]))
