#!/usr/bin/env python3
"""Decode-GEMM streaming bandwidth (M = 16 tokens, GPT-7B projections, bf16): each timed call
reads a different weight copy (8 copies rotate: no L2 / MALL reuse), TB/s of weight bytes per
config of skinny_linear_cfg (0 = automatic) and hipBLASLt.  ``--quant`` adds the quantised decode
weight streams of the fused path (M <= 16): ``fp8`` (decode_linear_fp8: e4m3fn + row scales) and
``int4`` (decode_linear_int4: group-128 int4 + group scales); their ``_tbs`` counts the bytes they
read (weights + scales), ``_us`` compares the formats.

    python tools/decode_gemm_bw.py [--configs 0 23 25] [--m 16 | --m 1 4 16] [--quant fp8 int4]
"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from llmctl.ops import _lib  # noqa: E402

SHAPES = {"qkv": (12288, 4096), "o": (4096, 4096), "up": (22016, 4096), "down": (4096, 11008), "lm": (32000, 4096)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[16])
    ap.add_argument("--quant", nargs="*", default=[], choices=["fp8", "int4"])
    ap.add_argument("--configs", type=int, nargs="+", default=[0, 23, 25])
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--knob", action="append", default=[])
    a = ap.parse_args()
    assert _lib.load(), _lib._error
    ops = torch.ops.llmctl
    for kv in a.knob:
        k, v = kv.split("=")
        ops.set_knob(k, int(v))
    from llmctl.ops.ref import dequant_int4_g128
    from llmctl.plugins.quantizers import quantize_fp8, quantize_int4_g128

    for name, (N, K) in SHAPES.items():
        ws = [(torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(a.copies)]
        # quantised copies: (qweight, scale) each from its own random weight, enough of them that a
        # cycle reads >= 768 MB (a 4096 x 4096 int4 weight is 8.5 MB: 8 copies would sit in the MALL);
        # the fp32 weight copy 0 stands for; bytes read per call
        quant = {}
        for fmt in a.quant:
            qf = quantize_fp8 if fmt == "fp8" else quantize_int4_g128
            nq, qs = a.copies, []
            while len(qs) < nq:
                d = qf(ws[len(qs)] if len(qs) < len(ws) else (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16))
                qs.append((d["qweight"].contiguous(), d["scale"].float().contiguous()))
                nbytes = sum(t.numel() * t.element_size() for t in qs[0])
                nq = max(a.copies, -(-768 * 2**20 // nbytes))
            wd = (qs[0][0].float() * qs[0][1].unsqueeze(1)) if fmt == "fp8" else dequant_int4_g128(*qs[0])
            quant[fmt] = (qs, wd, nbytes)
        for M in a.m:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            row = {"shape": name, "N": N, "K": K, "M": M}
            # (tag, call on copy i, fp32 reference of copy 0, bytes read per call, copies)
            ref = x.float() @ ws[0].float().t()
            runs = [(f"c{c}", lambda i, c=c: ops.skinny_linear_cfg(x, ws[i], None, c), ref, N * K * 2, a.copies)
                    for c in a.configs]
            runs.append(("hipblaslt", lambda i: torch.nn.functional.linear(x, ws[i]), ref, N * K * 2, a.copies))
            if M <= 16 and N % 64 == 0:
                for fmt, (qs, wd, nbytes) in quant.items():
                    op = ops.decode_linear_fp8 if fmt == "fp8" else ops.decode_linear_int4
                    runs.append((fmt, lambda i, op=op, qs=qs: op(x, qs[i][0], qs[i][1], None), x.float() @ wd.t(), nbytes,
                                 len(qs)))
            for tag, fn, want, nbytes, ncop in runs:
                iters = max(a.iters, ncop)
                row[tag + "_err"] = round(((fn(0).float() - want).abs().max() / want.abs().max()).item(), 5)
                # captured: a graph of `iters` back-to-back calls times the kernels, not the host
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for i in range(ncop):
                        fn(i)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for i in range(iters):
                        fn(i % ncop)
                g.replay()
                torch.cuda.synchronize()
                t = time.perf_counter()
                g.replay()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t) / iters
                row[tag + "_us"] = round(dt * 1e6, 1)
                row[tag + "_tbs"] = round(nbytes / dt / 1e12, 2)
                del g
            print(json.dumps(row), flush=True)
        del ws, quant


if __name__ == "__main__":
    main()
