"""The shared epilogue of the encoder bodies (csrc/ssd_policy_mfma.hip, enc_reduce_finish): the bias is one 16-byte load and the row's
output offset is formed in front of the reduction's barriers, the result is one 16-byte store per (row, 4 features) at any dword
address.  Launched through ssd_policy_encode on the class-LUT images:
  V = 15  k_encode_lut<15, *, 4>  (one band: writes `out`)
  V = 5   k_encode_lut_any        (one band: writes `out`)
  V = 21  k_encode_lut_any        (two bands: writes the band sums `part`, no bias)
  rows in {1, 63, 65, 200}: the `row < rows` guard in the first and in the last workgroup (64 rows per workgroup at V = 15, 80 else);
  agent_major 0 and 1 (n_agents 1, 3, 5, 5: rows must be a multiple);
  out_stride in {32, 35, 64}: ssd_policy_encode accepts every stride >= 32; 35 puts rows at dword addresses that are no multiple of 16
  bytes, and lin_b itself sits 4 bytes past a 16-byte boundary in that case.
Against the torch f32 encoder (Conv2d + LeakyReLU + Linear + LeakyReLU on the expanded planes, on the CPU) within the encoder tests'
2e-6; `out` / `part` live in a poisoned arena (tests/arena_util.py): the columns from 32 on, the bands around the operand and the slack
keep their fill, every element the contract writes is written."""
import ctypes as C

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from homophily_marl_amd import abi
from tests import arena_util as au

TOL = 2e-6
EDGES = (15, 5, 21)
ROWS = {1: 1, 63: 3, 65: 5, 200: 5}                 # rows -> n_agents
STRIDES = (32, 35, 64)
CASES = [(V, rows) for V in EDGES for rows in ROWS]


def test_case_list_covers_the_guard_and_both_paths():
    assert [abi.encode_bands(V) for V in EDGES] == [1, 1, 2]
    for V in EDGES:
        group = 64 if V == 15 else 80                # 16 BT rows per workgroup: BT = 4 at 15 x 15 (rows <= 32768), 5 for the run-time edge
        groups = sorted((r + group - 1) // group for r in ROWS)         # every last workgroup is ragged; one and several workgroups
        assert groups == ([1, 1, 2, 4] if V == 15 else [1, 1, 1, 3]) and all(r % group for r in ROWS)
    assert all(rows % n == 0 for rows, n in ROWS.items()) and any(s % 4 for s in STRIDES) and min(STRIDES) == 32


def _stream():
    return th.cuda.current_stream().cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("V,rows", CASES, ids=["V%d-rows%d" % c for c in CASES])
def test_encoder_tail_writes_what_the_torch_encoder_computes(V, rows):
    from homophily_marl_amd import ops
    lib = abi.load_library()
    n, O, bands = ROWS[rows], V - 2, abi.encode_bands(V)
    th.manual_seed(V * 1000 + rows)
    conv, lin = th.nn.Conv2d(3, 6, 3, 1), th.nn.Linear(6 * O * O, 32)
    g = th.Generator().manual_seed(rows * 100 + V)
    codes = th.randint(0, 4, (rows, V, V), generator=g).to(th.uint8)
    with th.no_grad():
        ref = F.leaky_relu(lin(F.leaky_relu(conv(ops.expand_codes(codes))).flatten(1))).numpy()       # [rows (env-major), 32]
    conv, lin = conv.cuda(), lin.cuda()
    codes_d = codes.cuda().contiguous()
    lb_store = th.zeros(36, device="cuda")
    cbytes, lbytes = abi.encode_frag_bytes(V, 2, abi.ENCODE_LAYOUT_LUT)
    table, frags = th.zeros(cbytes, dtype=th.uint8, device="cuda"), th.zeros(lbytes, dtype=th.uint8, device="cuda")
    abi.check(lib, lib.ssd_policy_pack_encoder_lut(conv.weight.data_ptr(), conv.bias.data_ptr(), lin.weight.data_ptr(), V, 2, table.data_ptr(),
                                                   frags.data_ptr(), _stream()))
    env = rows // n
    for agent_major in (0, 1):
        # output row of env-major row b * n + i
        orow = (np.arange(rows) % n) * env + np.arange(rows) // n if agent_major else np.arange(rows)
        for stride in (STRIDES if bands == 1 else (0,)):
            shift = 1 if stride % 4 else 0                               # lin_b at 4 bytes past a 16-byte boundary
            lb = lb_store[shift:shift + 32]
            lb.copy_(lin.bias.detach())
            assert lb.data_ptr() % 16 == 4 * shift
            ea = abi.SsdPolicyEncodeArgs()
            ea.codes, ea.code_bytes, ea.env_stride, ea.slot_stride, ea.agent_stride = codes_d.data_ptr(), codes_d.numel(), n * V * V, 0, V * V
            ea.rows, ea.view_edge, ea.n_agents, ea.agent_major, ea.precision = rows, V, n, agent_major, 2
            ea.alphabet, ea.layout = abi.CODE_CLASS, abi.ENCODE_LAYOUT_LUT
            ea.conv_frags, ea.lin_frags, ea.conv_b, ea.lin_b = table.data_ptr(), frags.data_ptr(), conv.bias.data_ptr(), lb.data_ptr()
            ar = au.Arena()
            if bands == 1:
                written = np.zeros((rows, stride), dtype=bool)
                written[:, :32] = True
                out = ar.reserve("out", (rows, stride), np.float32, align=16, offset_in_16=4 * shift, written=written)
                ea.out, ea.out_stride = out.ptr, stride
                assert (out.ptr % 16 == 0 and stride % 4 == 0) == (shift == 0)
            else:
                out = ar.reserve("part", (bands, rows, 32), np.float32, align=16)
                ea.part = out.ptr
            abi.check(lib, lib.ssd_policy_encode(C.byref(ea), _stream()))
            th.cuda.synchronize()
            ar.check()
            got = out.array()
            if bands == 1:
                feat = got[:, :32]
            else:                                                        # the env head's finish: LeakyReLU(lin_b + the band sums, band order)
                s = lin.bias.detach().cpu().numpy() + got.sum(axis=0, dtype=np.float32)
                feat = np.maximum(s, np.float32(0.01) * s)
            err = float(np.abs(feat[orow] - ref).max())
            print("V=%d rows=%d n=%d agent_major=%d out_stride=%d: max |diff| vs torch f32 %.2e" % (V, rows, n, agent_major, stride, err))
            assert err < TOL, (V, rows, agent_major, stride, err)
