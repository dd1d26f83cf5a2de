"""Replays: device-side recording of test episodes and the reference's replay figures (map_env.py:448-475, is_replay).

ReplayRecorder keeps the frames of an episode of selected envs on the device: frame k (the state after k steps, k = 0..T) is one
ssd_render launch into slot k of a [T + 1, k_envs, H, W, 3] buffer, the slot read from a device index (no host sync).  Positions,
incentive actions and rewards come from the episode batch at the end, and everything reaches the host in one copy per array.

write_replay draws, per recorded env, the reference's figure for every frame (imshow of the full-colour map with the agent legend,
title "step={k},collective={c}", and the incentive arrows of HomophilyMAC.select_actions_inc, controllers/homophily_controller.py:48-64):
<k>.png, frames.npz with the raw arrays and replay.gif.  The reference writes an mp4 with cv2 (make_video_from_image_dir); cv2 is
not a dependency here, so the video is an animated GIF written with PIL.
"""
import os
import time

import numpy as np
import torch

# DEFAULT_COLOURS['1'..'10'] (map_env.py:33-62): the legend of agent i uses str(i + 1) untruncated (map_env.py:466)
AGENT_LEGEND_RGB = [(159, 67, 255), (2, 81, 154), (204, 0, 204), (216, 30, 54), (254, 151, 0), (205, 155, 155), (99, 99, 255),
                    (250, 204, 255), (238, 223, 16), (0, 139, 139)]
# render classes of ssd_render: cell codes 0..5 (' ', '@', 'A', 'H', 'R', 'S'), 5 + agent char '1'..'9', 'F', 'C'
CELL_CHARS = " @AHRS"


def full_color_table(env):
    """color_map of the reference (DEFAULT_COLOURS, plus CLEANUP_COLORS for Cleanup) restricted to the chars a frame can hold:
    {char: (r, g, b)}."""
    t = {" ": (0, 0, 0), "@": (180, 180, 180), "A": (0, 255, 0), "F": (255, 255, 0)}
    for i, rgb in enumerate(AGENT_LEGEND_RGB[:9]):
        t[str(i + 1)] = rgb
    if env == "cleanup":
        t.update({"C": (100, 255, 255), "S": (113, 75, 24), "H": (99, 156, 194), "R": (113, 75, 24)})
    return t


def replay_dir(root):
    """<root>/replays/replay-<timestamp> (the reference's results/replays/ folder, one directory per run)."""
    return os.path.join(root, "replays", "replay-" + time.strftime("%Y-%m-%d_%H-%M-%S"))


class ReplayRecorder:
    """Frames [T + 1, k, H, W, 3] u8 of the envs `env_ids` of a render-mode env, on the device."""

    def __init__(self, native, env_ids, episode_limit):
        if not native.render_on:
            raise RuntimeError("ReplayRecorder needs an env in render mode (render=True or is_replay=True)")
        ids = [int(e) for e in env_ids]
        if not ids or min(ids) < 0 or max(ids) >= native.n_env:
            raise ValueError("replay_envs %s outside 0..%d" % (ids, native.n_env - 1))
        self.native, self.env_ids, self.T = native, ids, int(episode_limit)
        dev = native.device
        self.ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        self.ids_long = self.ids.long()
        self.frames = torch.zeros(self.T + 1, len(ids), native.H, native.W, 3, dtype=torch.uint8, device=dev)
        self.slots = torch.arange(self.T + 1, dtype=torch.int32, device=dev)   # slot k read by the kernel
        self.t = 0

    def begin(self):
        self.t = 0

    def frame(self):
        """Render the current state of the recorded envs as the next frame (after reset: frame 0; after step k: frame k)."""
        if self.t > self.T:
            raise RuntimeError("more than episode_limit + 1 frames in one episode")
        self.native.render_into(self.ids, self.frames, self.slots[self.t:self.t + 1])
        self.t += 1

    def finish(self, batch):
        """Host arrays of the episode: frames [k, T + 1, H, W, 3] u8, pos [k, T + 1, n, 2] (frame k's positions, row / col),
        actions_inc [k, T + 1, n, n] (chosen at runner step t), collective [k, T + 1] (env reward summed over agents and the
        steps before frame k)."""
        ids = self.ids_long
        pos = batch["agent_pos"][ids].float()
        inc = batch["actions_inc"][ids].reshape(len(self.env_ids), self.T + 1, pos.shape[2], pos.shape[2]).to(torch.int32)
        rew = batch["reward"][ids].reshape(len(self.env_ids), self.T + 1, -1)[:, :self.T].sum(-1)
        coll = torch.cat([torch.zeros_like(rew[:, :1]), torch.cumsum(rew, 1)], 1).float()
        out = dict(frames=self.frames[:self.t].transpose(0, 1), pos=pos, actions_inc=inc, collective=coll)
        return {k: v.contiguous().cpu().numpy() for k, v in out.items()}


def _figure(rgb, step, collective, env_name, n_agents, pos=None, incentives=None):
    from matplotlib.figure import Figure
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    import matplotlib.patches as mpatches
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(111)
    if incentives is not None:         # drawn before the map, as the controller's arrows are (homophily_controller.py:48-64)
        for i in range(n_agents):
            for j in range(n_agents):
                if i != j and incentives[i, j] != 0:
                    ax.arrow(x=pos[i, 1] + 0.2, y=pos[i, 0] + 0.2, dx=pos[j, 1] - pos[i, 1] - 0.2, dy=pos[j, 0] - pos[i, 0] - 0.2,
                             alpha=0.8, width=0.1, head_width=0.8, color="lime" if incentives[i, j] == 1 else "deepskyblue")
    ax.imshow(rgb, interpolation="nearest")
    patch = [mpatches.Patch(color=np.array(AGENT_LEGEND_RGB[i]) / 256, label=str(i)) for i in range(n_agents)]
    if env_name == "harvest":
        ax.legend(handles=patch, loc="upper center", bbox_to_anchor=(0.5, -0.1), ncol=min(5, n_agents))
    else:
        ax.legend(handles=patch, loc="lower left", bbox_to_anchor=(1.05, 0), ncol=1)
    ax.set_title("step={},collective={}".format(step, int(collective)))
    return fig


def write_frame_png(path, rgb, step, collective, env_name, n_agents, pos=None, incentives=None):
    _figure(rgb, step, collective, env_name, n_agents, pos, incentives).savefig(path)


def write_gif(png_paths, path, duration_ms=100):
    from PIL import Image
    imgs = [Image.open(p).convert("RGB") for p in png_paths]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=duration_ms, loop=0)
    return path


def write_replay(out_dir, rec, env_name, env_ids=None, gif=True):
    """Per recorded env e: <out_dir>/env_<e>/<k>.png for k = 0..T, frames.npz and replay.gif.  `rec` is ReplayRecorder.finish().
    Frame k >= 2 carries the incentive arrows chosen at runner step k - 1, drawn from the positions of frame k."""
    frames = rec["frames"]
    k_envs, n_frames = frames.shape[:2]
    env_ids = list(range(k_envs)) if env_ids is None else list(env_ids)
    n = rec["pos"].shape[2]
    dirs = []
    for i, e in enumerate(env_ids):
        d = os.path.join(out_dir, "env_%d" % e)
        os.makedirs(d, exist_ok=True)
        pngs = []
        for k in range(n_frames):
            inc = rec["actions_inc"][i, k - 1] if k >= 2 else None
            p = os.path.join(d, "%d.png" % k)
            write_frame_png(p, frames[i, k], k, rec["collective"][i, k], env_name, n, rec["pos"][i, k], inc)
            pngs.append(p)
        np.savez_compressed(os.path.join(d, "frames.npz"), frames=frames[i], pos=rec["pos"][i], actions_inc=rec["actions_inc"][i],
                            collective=rec["collective"][i])
        if gif:
            write_gif(pngs, os.path.join(d, "replay.gif"))
        dirs.append(d)
    return dirs
