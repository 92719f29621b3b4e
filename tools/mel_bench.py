"""Times of the one-launch log-mel analysis (csrc/melspec.hip), for DESIGN.md section 12:

  * l2s_mel_spectrogram at the headline batch (640 clips x 64 000 samples, int16 and fp32) and at one clip;
  * yardstick (a), same process: the fp32 tap-GEMM on the equivalent LINEAR problem (M = 640 * 401 pre-framed rows, N = K = 640,
    the packed basis as the weight) - the one-launch kernel should not take more than that GEMM alone;
  * yardstick (b), tool only: torch.stft + matmul + log on the same device (the library route the charter keeps out of product
    code), with the largest difference between the two results;
  * for DESIGN.md section 16, l2s_stft_mel at the loss's sizes (1024 / 256, pad 384): a validation batch (16 x 8 960 samples)
    and the headline batch (640 x 64 000 samples), each beside the fp32 tap-GEMM on its pre-framed LINEAR problem
    (N = K = 1024), same process.

  python tools/mel_bench.py [--steps 20] [--batch 640] [--samples 64000]

Each figure is the median of `steps` timed runs between HIP events after 3 warm-up runs, with the min - max spread."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.f32_bench import timed  # noqa: E402

PEAK_F32_MATRIX = 157.3e12     # v_mfma_f32_32x32x2_f32: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def loss_sizes(steps):
    """l2s_stft_mel at (1024, 256, pad 384, eps 1e-9) against the f32 tap-GEMM on the pre-framed frames."""
    from lip2speech_unit_amd import audio, ops
    ms = audio.MelSpectrogram()
    g = torch.Generator().manual_seed(1)
    for B, S in ((16, 8960), (640, 64000)):
        T = ms.num_frames(S)
        wav = (torch.randint(-20000, 20000, (B, S), generator=g, dtype=torch.int16).float() / 32768.0).cuda()
        basis, fb, rng = ms.tables(wav.device)
        mel = torch.empty(B, T, 80, device="cuda")
        fl = 2.0 * B * T * 1024 * 1024
        med, lo, hi = timed(lambda: ops.stft_mel(wav, mel, basis, fb, rng, B=B, S=S, T_rows=T, n_fft=1024, hop=256, pad=ms.pad,
                                                 mag_eps=ms.mag_eps), steps)
        print(f"stft_mel 1024/256 fp32 B{B} S{S} ({T} frames): {med * 1e3:9.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}) = "
              f"{fl / med / 1e9:6.1f} TFLOP/s = {100 * fl / med / 1e-3 / PEAK_F32_MATRIX:.1f} % of the f32 matrix peak", flush=True)
        M = B * T
        frames = torch.nn.functional.pad(wav[:, None], (ms.pad, ms.pad), mode="reflect")[:, 0].unfold(1, 1024, 256).reshape(M, 1024).contiguous()
        W = basis.t().contiguous()
        C = torch.empty(M, 1024, device="cuda")
        gm, glo, ghi = timed(lambda: ops.tapgemm(frames, W, C, M=M, N=1024, Cin=1024, dtype=ops.F32), steps)
        print(f"    tapgemm f32 LINEAR M{M} N1024 K1024 (pre-framed): {gm * 1e3:9.1f} us (min {glo * 1e3:.1f}, max {ghi * 1e3:.1f}) = "
              f"{fl / gm / 1e9:6.1f} TFLOP/s; one-launch mel / GEMM alone = {med / gm:.2f}", flush=True)
        del frames, C, wav, mel
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=640)
    ap.add_argument("--samples", type=int, default=64000)
    a = ap.parse_args()
    from lip2speech_unit_amd import audio, ops
    st = audio.TacotronSTFT()
    g = torch.Generator().manual_seed(0)
    B, S = a.batch, a.samples
    T = audio.num_frames(S)
    pcm = torch.randint(-20000, 20000, (B, S), generator=g, dtype=torch.int16).cuda()
    wav = pcm.float() / 32768.0
    basis, fb, rng = st.tables(pcm.device)
    mel = torch.empty(B, T, 80, device="cuda")
    fl = 2.0 * B * T * 640 * 640
    for tag, x in (("int16", pcm), ("fp32", wav)):
        med, lo, hi = timed(lambda: ops.mel_spectrogram(x, mel, basis, fb, rng, B=B, S=S, T_rows=T), a.steps)
        print(f"mel_spectrogram {tag} B{B} S{S} ({T} frames): {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}) = {fl / med / 1e9:6.1f} TFLOP/s "
              f"= {100 * fl / med / 1e-3 / PEAK_F32_MATRIX:.1f} % of the f32 matrix peak", flush=True)
    mel_med = med
    one = pcm[:1].contiguous()
    mel1 = torch.empty(1, T, 80, device="cuda")
    med, lo, hi = timed(lambda: ops.mel_spectrogram(one, mel1, basis, fb, rng, B=1, S=S, T_rows=T), a.steps)
    print(f"mel_spectrogram int16 B1 S{S}: {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
    # (a) the GEMM alone on a pre-framed matrix
    M = B * T
    frames = torch.nn.functional.pad(wav[:, None], (320, 320), mode="reflect")[:, 0].unfold(1, 640, 160).reshape(M, 640).contiguous()
    W = basis.t().contiguous()                     # tapgemm weights are [N, K]
    C = torch.empty(M, 640, device="cuda")
    med, lo, hi = timed(lambda: ops.tapgemm(frames, W, C, M=M, N=640, Cin=640, dtype=ops.F32), a.steps)
    print(f"(a) tapgemm f32 LINEAR M{M} N640 K640 (pre-framed): {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}) = {fl / med / 1e9:6.1f} TFLOP/s; "
          f"one-launch mel / GEMM alone = {mel_med / med:.2f}", flush=True)
    del frames, C
    torch.cuda.empty_cache()
    # (b) the library route
    win = torch.hann_window(640, periodic=True, device="cuda")

    def lib_route():
        spec = torch.stft(wav, 640, hop_length=160, win_length=640, window=win, center=True, pad_mode="reflect", return_complex=True)
        return torch.log(torch.clamp(torch.matmul(fb, spec.abs()), min=1e-5)).transpose(1, 2)
    med, lo, hi = timed(lib_route, a.steps)
    diff = (lib_route() - mel).abs().max().item()
    print(f"(b) torch.stft + matmul + log, same device: {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}); one-launch mel / library route = "
          f"{mel_med / med:.2f}; max |difference| {diff:.2e}", flush=True)
    del wav, pcm, mel
    torch.cuda.empty_cache()
    loss_sizes(a.steps)


if __name__ == "__main__":
    main()
