"""``DeviceNoise``: the Gaussian noise of a generation drawn ON the device by ``pd_stream_noise``, from the counter-based stream
``include/phendiff_hip.h`` defines (Philox4x32-10 + Box-Muller, the stream of ``pd_train_sample``), at a position that lives in device
memory.  One stream per IMAGE: image ``k`` of a run draws with step ``k``, so what it gets depends on ``(seed, k)`` alone -- not on the
batch size, the rank layout or the batches drawn before it -- and a captured trajectory whose last node is ``pd_stream_advance`` draws
the next images on its next replay (:class:`~phendiff_amd.trajectories.GenerationGraph`).

It is NOT torch's CPU stream and NOT torch's device Philox layout: a run that must reproduce a ``torch.Generator``'s draws passes that
generator, as before."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

STEP_LIMIT = 1 << 48      # the counter's step field


class DeviceNoise:
    """``DeviceNoise(seed, device, rank=0, first_index=0)`` owns the 16-byte device state ``{seed, index}`` and a host shadow of
    ``index``, the global number of the next image.  Row ``b`` of every draw belongs to image ``index + b``:

      * ``randn(shape, purpose)``: standard normals, ``(B, ...)``;
      * ``add_noise(scheduler, x, timesteps)``: ``DDIMScheduler.add_noise`` with the images' forward noise, one launch;
      * ``variance_noise(i, shape)``: the variance noise of trajectory step ``i`` (``eta > 0``); ``add_variance_noise`` adds it in place;
      * ``advance(n)`` moves on by ``n`` images, ``seek(index)`` goes to image ``index``; ``state_dict`` / ``load_state_dict`` resume.

    Draws do not advance the position (an image's initial sample, forward noise and variance noise all belong to the same index):
    whoever finishes a batch advances by its size.  Everything is enqueued on torch's current stream unless a stream is given."""

    PURPOSE_RANDN = 2      # pd_train_sample's "a plain randn"
    PURPOSE_INITIAL_SAMPLE = L.CONSTANTS["PD_PURPOSE_INITIAL_SAMPLE"]
    PURPOSE_FORWARD_NOISE = L.CONSTANTS["PD_PURPOSE_FORWARD_NOISE"]
    PURPOSE_VARIANCE_NOISE = L.CONSTANTS["PD_PURPOSE_VARIANCE_NOISE"]

    def __init__(self, seed: int, device, rank: int = 0, first_index: int = 0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.PhenDiffHipError("DeviceNoise draws on MI355X only (no CPU fallback)")
        if not 0 <= int(rank) < 4096:
            raise ValueError(f"DeviceNoise: rank {rank} outside [0, 4096)")
        self.seed, self.rank = int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank)
        self._index = self._checked(first_index)
        self.state = torch.tensor([self._signed(self.seed), self._index], dtype=torch.int64).to(self.device)

    @staticmethod
    def _signed(v: int) -> int:
        return v - (1 << 64) if v >= 1 << 63 else v

    @staticmethod
    def _checked(index, rows: int = 0) -> int:
        index = int(index)
        if index < 0 or index + rows > STEP_LIMIT:
            raise ValueError(f"DeviceNoise: image index {index} (+ {rows} rows) outside the counter's step field [0, 2^48]")
        return index

    @property
    def index(self) -> int:
        """The host shadow of the device index: the global number of the next image."""
        return self._index

    # ---- position ---------------------------------------------------------------------------------------------------------------------
    def seek(self, index: int):
        """Go to image ``index`` (stream-ordered on torch's current stream, like every draw)."""
        self._index = self._checked(index)
        self.state.copy_(torch.tensor([self._signed(self.seed), self._index], dtype=torch.int64), non_blocking=False)
        return self

    def advance(self, n: int, stream=None):
        """``index += n`` on the device (one ``pd_stream_advance`` launch) and in the shadow."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        self._checked(self._index, int(n))
        L.check(L.lib().pd_stream_advance(self.state.data_ptr(), int(n), st), "pd_stream_advance")
        self._index += int(n)
        return self

    def note_advanced(self, n: int):
        """The shadow's half of ``advance``: a captured ``pd_stream_advance`` has been (or is about to be) replayed."""
        self._index = self._checked(self._index + int(n))

    def state_dict(self) -> dict:
        return {"seed": self.seed, "rank": self.rank, "index": self._index}

    def load_state_dict(self, sd: dict):
        self.seed, self.rank = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF, int(sd["rank"])
        return self.seek(int(sd["index"]))

    # ---- launches ---------------------------------------------------------------------------------------------------------------------
    def launch_args(self, out, B: int, per_sample: int, purpose: int, x=None, a: float = 1.0, b: float = 1.0, sa=None, sb=None,
                    elem_base: int = 0, index_offset: int = 0) -> "L.StreamNoiseArgs":
        """The ``pd_stream_noise`` argument struct of ``out = a x + b z`` (``sa`` / ``sb``: per-row tables instead of the scalars) over
        ``[B][per_sample]``.  Buffers are dense fp32 tensors or raw device pointers; the struct points at this object's state, so the
        launch -- captured or not -- draws at whatever position the state holds when it runs."""
        ptr = lambda t: t.data_ptr() if torch.is_tensor(t) else t
        return L.StreamNoiseArgs(state=self.state.data_ptr(), index_offset=int(index_offset), rank=self.rank, purpose=int(purpose),
                                 B=int(B), per_sample=int(per_sample), elem_base=int(elem_base), a=float(a), b=float(b),
                                 sa=ptr(sa), sb=ptr(sb), x=ptr(x), out=ptr(out))

    def enqueue(self, args: "L.StreamNoiseArgs", stream=None):
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        self._checked(self._index + args.index_offset, args.B)
        L.check(L.lib().pd_stream_noise(C.byref(args), st), "pd_stream_noise")

    def _on_device(self, t, what):
        if not t.is_cuda or t.device != self.device:
            raise L.PhenDiffHipError(f"DeviceNoise: {what} must live on {self.device} (no CPU fallback)")

    @torch.no_grad()
    def randn(self, shape, purpose: int = PURPOSE_RANDN, elem_base: int = 0, index_offset: int = 0) -> torch.Tensor:
        """Standard normals of shape ``(B, ...)``: row ``b`` is elements ``elem_base ..`` of image ``index + index_offset + b``'s stream
        under ``purpose``."""
        shape = tuple(int(v) for v in shape)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self.enqueue(self.launch_args(out, shape[0], out[0].numel(), purpose, a=0.0, b=1.0, elem_base=elem_base,
                                      index_offset=index_offset))
        return out

    @torch.no_grad()
    def add_noise(self, scheduler, x: torch.Tensor, timesteps: torch.Tensor, elem_base: int = 0) -> torch.Tensor:
        """``scheduler.add_noise(x, z, timesteps)`` with ``z`` the images' forward noise, drawn inside the launch.  ``elem_base``: where in
        each image's forward-noise stream the draw starts (draw ``k`` of several noisings of one image: ``k * per_sample``)."""
        self._on_device(x, "x")
        x = x.contiguous().float()
        B = x.shape[0]
        if timesteps.numel() == 1:
            timesteps = timesteps.reshape(1).expand(B)
        sa, sb = scheduler._per_sample_coefs(timesteps, x.device)
        out = torch.empty_like(x)
        self.enqueue(self.launch_args(out, B, x[0].numel(), self.PURPOSE_FORWARD_NOISE, x=x, sa=sa, sb=sb, elem_base=elem_base))
        return out

    def variance_noise(self, i: int, shape) -> torch.Tensor:
        """The variance noise of trajectory step ``i`` (its position in the scheduler's timesteps): elements ``i * per_sample ..`` of every
        image's stream under the variance purpose."""
        shape = tuple(int(v) for v in shape)
        per = 1
        for v in shape[1:]:
            per *= v
        return self.randn(shape, self.PURPOSE_VARIANCE_NOISE, elem_base=int(i) * per)

    def variance_args(self, i: int, sample, sigma: float, B: int = None, per_sample: int = None) -> "L.StreamNoiseArgs":
        """``sample += sigma * variance_noise(i)`` in place, as one launch's arguments."""
        if B is None:
            B, per_sample = sample.shape[0], sample[0].numel()
        return self.launch_args(sample, B, per_sample, self.PURPOSE_VARIANCE_NOISE, x=sample, a=1.0, b=float(sigma),
                                elem_base=int(i) * per_sample)

    def add_variance_noise(self, sample: torch.Tensor, sigma: float, i: int, stream=None) -> torch.Tensor:
        self._on_device(sample, "sample")
        self.enqueue(self.variance_args(i, sample, sigma), stream)
        return sample
