"""Episode videos from device-side envs: frames drawn by fa_render into one device buffer, cut into episodes on the host.

The reference's evaluation scripts render every step of their one env (test_fortattack.py --render --record
--video-format gif).  Here `EpisodeRecorder` records K chosen envs of a handle of thousands: after every step of a chunk
`BatchedFortAttack.render` (csrc/fa_render.hip) draws their frames straight from the device state into slot s + 1 of a
(num_steps + 1, K, size, size, 3) buffer -- a fixed pointer per slot, so the launches sit inside the hipGraph that plays
the chunk -- and `end_chunk` brings the chunk's frames and the K envs' done flags to the host.  `split_episodes` is the
pure-numpy part: frames + done flags -> per env a list of episodes.

Frame t + 1 shows the state AFTER step t with the lasers and attention of step t.  With auto-reset the step kernel has
already reset an env whose episode ended, so the frame after an episode's last step is the next episode's reset frame (drawn
without lasers); the terminal state itself is never seen -- as in the reference's own Learner loop, which never stores that
observation either.  The episode's outcome is in the cross-play table.
"""
import numpy as np

MAX_DEVICE_BYTES = 2 << 30


def split_episodes(frames, done, episodes_per_env):
    """frames (S + 1, K, size, size, 3): frame 0 the reset frame, frame s + 1 the one drawn after step s; done (S, K): step s
    ended an episode of recorded env k.  Returns, per recorded env, a list of at most `episodes_per_env` arrays
    (L, size, size, 3), L = the episode's number of steps: an episode starts at its reset frame -- frame 0, or the frame drawn
    after the step that ended the episode before (a step with `done` set contributes the NEXT episode's first frame) -- and
    runs up to the frame before its own last step's.  Frames past the quota are dropped, and so is a trailing episode that has
    not ended within the S steps: every returned episode is whole."""
    frames, done = np.asarray(frames), np.asarray(done) != 0
    if frames.ndim != 5 or done.ndim != 2 or frames.shape[0] != done.shape[0] + 1 or frames.shape[1] != done.shape[1]:
        raise ValueError("split_episodes: frames (S + 1, K, size, size, 3) and done (S, K) expected, got %s and %s"
                         % (frames.shape, done.shape))
    out = []
    for k in range(frames.shape[1]):
        episodes, start = [], 0
        for s in np.nonzero(done[:, k])[0]:
            if len(episodes) == int(episodes_per_env):
                break
            episodes.append(frames[start:s + 1, k].copy())
            start = s + 1
        out.append(episodes)
    return out


def write_npz(path, episodes):
    """One env's episodes -> path: arrays ep0, ep1, ... of (L, size, size, 3) uint8 (np.load(path)["ep0"])."""
    np.savez_compressed(path, **{"ep%d" % i: np.asarray(ep, np.uint8) for i, ep in enumerate(episodes)})


def write_gif(path, frames, fps=10):
    """(L, size, size, 3) uint8 -> an endlessly looping GIF through PIL.  (PIL merges consecutive frames that are identical
    into one of a longer duration: the file then holds fewer than L images, and plays the same.)"""
    try:
        from PIL import Image
    except ImportError as exc:
        raise RuntimeError("write_gif needs PIL (the Pillow package), which cannot be imported: %s; "
                           "record with --video-format npz instead" % exc)
    frames = np.asarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.shape[0] < 1:
        raise ValueError("write_gif: (L, size, size, 3) frames expected, got %s" % (frames.shape,))
    imgs = [Image.fromarray(np.ascontiguousarray(f)) for f in frames]
    imgs[0].save(path, format="GIF", save_all=True, append_images=imgs[1:], duration=max(int(round(1000.0 / fps)), 10), loop=0)


class EpisodeRecorder(object):
    """EpisodeRecorder(eng, env_index, num_steps): records envs `env_index` of the BatchedFortAttack `eng` over chunks of
    `num_steps` steps.  capture_reset() after the reset, capture(s, storage, attn_out) after step s, end_chunk(storage) after
    the chunk; then frames() / done() / episodes(n)."""

    def __init__(self, eng, env_index, num_steps, size=128, viz_dead=False, viz_attn=True):
        idx = np.asarray(env_index)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
            raise ValueError("EpisodeRecorder: env_index must be a non-empty 1-d integer sequence")
        if int(idx.min()) < 0 or int(idx.max()) >= eng.E:
            raise ValueError("EpisodeRecorder: env_index must lie in [0, %d)" % eng.E)
        self.T, self.K, self.size = int(num_steps), int(idx.size), int(size)
        if self.T < 1:
            raise ValueError("EpisodeRecorder: num_steps must be >= 1")
        nbytes = (self.T + 1) * self.K * self.size * self.size * 3
        if nbytes > MAX_DEVICE_BYTES:
            raise ValueError("EpisodeRecorder: the frame buffer of (%d + 1) steps x %d envs x %d x %d x 3 would take %.2f GiB "
                             "of device memory (limit 2 GiB): record fewer envs, smaller frames or shorter chunks"
                             % (self.T, self.K, self.size, self.size, nbytes / float(1 << 30)))
        import torch
        self.eng, self.viz_dead, self.viz_attn = eng, bool(viz_dead), bool(viz_attn)
        self.env_index = idx.astype(np.int64)
        self._idx = torch.from_numpy(idx.astype(np.int32)).to(eng.device)
        self._idx_long = self._idx.long()
        self.buf = torch.zeros((self.T + 1, self.K, self.size, self.size, 3), dtype=torch.uint8, device=eng.device)
        self._frames, self._done = [], []

    def capture_reset(self):
        """Slot 0 <- the state as it is (call after the reset that starts the recording); forgets earlier chunks."""
        self._frames, self._done = [], []
        self.eng.render(self._idx, self.size, viz_dead=self.viz_dead, viz_attn=False, out=self.buf[0])

    def capture(self, s, storage, attn_out=None):
        """Slot s + 1 <- the state after step s: lasers from storage.actions[s], none where storage.done[s] is set (that env
        already shows its next episode's reset state), attention from attn_out[0], the guards' maps of that step's forward."""
        self.eng.render(self._idx, self.size, actions=storage.actions[s], no_laser=storage.done[s],
                        attn=None if attn_out is None else attn_out[0], viz_dead=self.viz_dead, viz_attn=self.viz_attn,
                        out=self.buf[s + 1])

    def end_chunk(self, storage):
        """The chunk's frames and the recorded envs' done flags -> host; the last slot becomes slot 0 of the next chunk."""
        first = 0 if not self._frames else 1          # slot 0 of a later chunk is the chunk before's last frame
        self._frames.append(self.buf[first:].cpu().numpy())
        self._done.append(storage.done[:self.T].index_select(1, self._idx_long).cpu().numpy())
        self.buf[0].copy_(self.buf[self.T])

    def frames(self):
        """(1 + steps recorded, K, size, size, 3) uint8."""
        return np.concatenate(self._frames, 0) if self._frames else np.zeros((0, self.K, self.size, self.size, 3), np.uint8)

    def done(self):
        """(steps recorded, K) uint8."""
        return np.concatenate(self._done, 0) if self._done else np.zeros((0, self.K), np.uint8)

    def episodes(self, episodes_per_env):
        """split_episodes over everything recorded since capture_reset()."""
        return split_episodes(self.frames(), self.done(), episodes_per_env)
