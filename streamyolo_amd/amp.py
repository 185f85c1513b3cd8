"""Dynamic loss scaling for the fused training path, device-resident (no host read anywhere in an iteration).

What `self.scaler = torch.cuda.amp.GradScaler(enabled=args.fp16)` does around the reference's optimizer step
(exps/train_utils/double_trainer.py:113-119: `scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()`), for
`TrainStep.step(x, targets, scaler)` + `FusedSGDEMA.step(lr, scaler=scaler)`: the scale, the growth tracker and the found-inf flag
live in one 32-byte device struct (sy_scaler_state, include/streamyolo_hip.h) that the kernels read through a pointer, so launch
tapes and captured graphs see each iteration's scale.  The drop-in autograd path keeps using torch.amp.GradScaler itself."""
import torch

from . import _lib, ops


class DeviceGradScaler:
    """torch.amp.GradScaler's rule (same defaults, same state_dict keys: a checkpoint written by either loads into the other).

    An iteration: `step.step(x, targets, scaler)` leaves `scale x` gradients; `opt.step(lr, scaler=scaler)` looks for inf / nan
    (sy_grad_nonfinite), applies the unscaled update unless one was found (sy_sgd_ema_step_scaled) and then grows / backs off the
    scale (sy_loss_scale_update).  get_scale() / found_inf() / counters() read the device state and therefore SYNCHRONISE: they
    are for logging and tests, not for the training loop."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        assert growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) > 0
        self.enabled = bool(enabled)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._init = (float(init_scale), 0)                      # (scale, growth tracker) until the state exists on a device
        self._state = None

    # ---- device state ----------------------------------------------------------------------------------------------------
    def state(self, device):
        """The sy_scaler_state tensor (8 x int32) on `device`, created at first use as GradScaler creates its scale lazily."""
        device = torch.device(device)
        if self._state is None:
            self._state = torch.zeros(8, dtype=torch.int32, device=device)
            self._write(*self._init)
        assert self._state.device == device, "DeviceGradScaler: one scaler serves one device"
        return self._state

    def _write(self, scale, tracker):
        s = _lib.ScalerState()
        s.scale, s.growth_tracker = scale, tracker
        s.inv_scale = float(torch.tensor(s.scale, dtype=torch.float64).reciprocal().float())     # GradScaler.unscale_'s rounding
        raw = torch.frombuffer(bytearray(bytes(s)), dtype=torch.int32)
        self._state[:4].copy_(raw[:4])                           # scale, inv_scale, tracker, found_inf = 0; the counters stay

    def _read(self):
        if self._state is None:
            s = _lib.ScalerState()
            s.scale, s.growth_tracker = self._init
            return s
        return _lib.ScalerState.from_buffer_copy(self._state.cpu().numpy().tobytes())

    # ---- launches (no host read) ------------------------------------------------------------------------------------------
    def check_gradients(self, table, n_entries, total_chunks):
        """found_inf |= any inf / nan among the gradients of a sy_optim_entry table (device tensor), on the current stream."""
        _lib.check(_lib.lib().sy_grad_nonfinite(table.data_ptr(), n_entries, total_chunks, self.state(table.device).data_ptr(),
                                                ops.stream_of(table)), "sy_grad_nonfinite")

    def update(self):
        """GradScaler.update(): back off after a found inf / nan, grow after `growth_interval` clean iterations; clears the flag."""
        st = self._state
        assert st is not None, "DeviceGradScaler.update before any scaled step"
        _lib.check(_lib.lib().sy_loss_scale_update(st.data_ptr(), self.growth_factor, self.backoff_factor, self.growth_interval,
                                                   ops.stream_of(st)), "sy_loss_scale_update")

    # ---- host-side read-outs (synchronise) --------------------------------------------------------------------------------
    def get_scale(self):
        """The current loss scale.  Synchronises (device -> host copy)."""
        return float(self._read().scale) if self.enabled else 1.0

    def found_inf(self):
        """Whether the check of the current iteration has found an inf / nan (cleared by update()).  Synchronises."""
        return bool(self._read().found_inf)

    def counters(self):
        """{"steps_taken", "steps_skipped", "growth_tracker"} since construction.  Synchronises."""
        s = self._read()
        return {"steps_taken": int(s.steps_taken), "steps_skipped": int(s.steps_skipped), "growth_tracker": int(s.growth_tracker)}

    def state_dict(self):
        """torch.amp.GradScaler.state_dict()'s keys and meaning ({} when disabled).  Synchronises."""
        if not self.enabled:
            return {}
        s = self._read()
        return {"scale": float(s.scale), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(s.growth_tracker)}

    def load_state_dict(self, state_dict):
        if not self.enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self.growth_factor, self.backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self.growth_interval = int(state_dict["growth_interval"])
        self._init = (float(state_dict["scale"]), int(state_dict["_growth_tracker"]))
        if self._state is not None:
            self._write(*self._init)

