"""CPU: ``vtaco_amd.ops`` as a package keeps the surface the single module had.

SURFACE was recorded from the single-module ``vtaco_amd/ops.py`` (the commit before the split), never from the tree under test: every
attribute that is a function or class of this project or an upper-case constant, plus the underscore names other code reaches through
``ops.`` (``_c``, ``_cl_storage``, ``_lib``, ``_mc_guess``).  Callables carry ``str(inspect.signature(...))`` (None where Python gives none),
constants their ``repr``."""
import inspect
import os
import re
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SURFACE = {'EMD_EPS_FINAL': ('const', '1e-06'),
 'EMD_MAX_POINTS': ('const', '4096'),
 'EMD_MAX_ROUNDS': ('const', '500000'),
 'EmdResult': ('callable', '(emd, assign, prices, rounds, bids, phases, eps)'),
 'FUSION_TENSORS': ('const', "('WK', 'WQ', 'WV', 'trans_conv', 'linear1_w', 'linear1_b', 'linear2_w', 'linear2_b', 'norm2_w', 'norm2_b')"),
 'GRID_SCATTER_SORTED': ('const', 'True'),
 'I32': ('const', 'torch.int32'),
 'MANO_BLOB_FLOATS': ('const', '330240'),
 'MISE_MAX_N': ('const', '513'),
 'PLANES': ('const', "{'xz': 0, 'xy': 1, 'yz': 2}"),
 'PRECISIONS': ('const', "('f32', 'bf16x3', 'f16x3', 'f16f8')"),
 'PlaneIndex': ('callable', "(pts, reso, padding=0.1, plane='xz')"),
 'RANGE_FP8': ('const', '2'),
 'RANGE_HALF': ('const', '1'),
 'RANGE_LOGIT': ('const', '4'),
 'SPLIT_PRECISIONS': ('const', "('bf16x3', 'f16x3', 'f16f8')"),
 'TOUCH_MAX_ROWS': ('const', '254'),
 'TactileUnetTrainWorkspace': ('callable', '(buf)'),
 'U8': ('const', 'torch.uint8'),
 'VoxelIndex': ('callable', '(pts, reso, padding=0.1, clear=None, want_tile_flags=False)'),
 'VtError': ('callable', None),
 'WIDE_SLICE': ('const', '524288'),
 '_c': ('callable', '(t)'),
 '_cl_storage': ('callable', '(grid)'),
 'blob_floats': ('callable', '(hidden=32, c_dim=32, n_blocks=5)'),
 'chamfer_nn': ('callable', '(a, b)'),
 'channel_stats': ('callable', '(x)'),
 'check': ('callable', '(rc, what)'),
 'contact_points': ('callable', '(depth, index, sel, kept, row0, pose, width, height, fov, max_points, p_sample, finger=None)'),
 'contact_scan': ('callable', '(depth, origin, touch, threshold=0.0001)'),
 'conv1x1_bwd_masked': ('callable', '(dout, y, w, want_dw=True, want_db=True)'),
 'conv1x1_cl': ('callable', '(x, weight, bias)'),
 'conv1x1_pack_f16x3': ('callable', '(weight)'),
 'conv3d_dgrad_xstats': ('callable', '(g, packed_t, Cin, g_absmax, x)'),
 'conv3d_gcr': ('callable',
                '(x, low, ss, packed_w, Cout, relu=True, packed_w_bf16x3=None, want_stats=True, packed_w_f16x3=None, in_absmax=None, '
                'thin_half=False, packed_w_up=None)'),
 'conv3d_gcr_final': ('callable', '(x, ss, packed_w_f16x3, final_packed, final_bias)'),
 'conv3d_gcr_final_keep': ('callable', '(x, ss, packed_w_f16x3, final_packed, final_bias)'),
 'conv3d_gcr_skip': ('callable', '(x, ss, packed_w_f16x3, Cout, tile_flags, relu=True)'),
 'conv3d_pack': ('callable', "(weight, precision='f32')"),
 'conv3d_pack_t': ('callable', '(weight)'),
 'conv3d_pack_up': ('callable', '(weight, c_skip)'),
 'conv3d_skip_covers': ('callable', '(x, Cout)'),
 'conv3d_up_covers': ('callable', '(C1, C2, B, D, H, W, Cout)'),
 'conv3d_wgrad': ('callable', "(x, low, ss, g, precision='f32', g_absmax=None)"),
 'conv3d_wgrad_sparse': ('callable', '(x, ss, g, tile_flags, g_absmax=None)'),
 'decode_bwd': ('callable',
                '(grid_shape, blob_t, grad_out, save, pts=None, lattice=None, with_c_img=False, c_img=None, padding=0.1, want_grid_grad=True, '
                'grad_out2=None)'),
 'decode_bwd_wide': ('callable',
                     '(grid_shape, blob_t, grad_out, save, pts, hidden, nb, leaky, nearest, padding=0.1, c_img=None, want_grid_grad=True, '
                     'grad_out2=None, want_rows=False)'),
 'decode_fwd': ('callable',
                "(grid, blob, pts=None, c_img=None, padding=0.1, lattice=None, want_contact=False, out=None, save=None, precision='f32', wide=None, "
                'finger_ids=None, finger_feats=None)'),
 'decode_fwd_ids': ('callable', "(grid, blob, ids, feats, pts=None, lattice=None, padding=0.1, out=None, precision='f32')"),
 'decode_fwd_wide_train': ('callable', '(grid, blob, pts, c_img, hidden, nb, leaky, nearest, padding=0.1, want_contact=False)'),
 'decode_last_clock': ('callable', '(workgroups=False)'),
 'decode_mlp_bwd': ('callable', '(blob_t, grad_out, save, pts, C=32)'),
 'decode_mlp_bwd_wide': ('callable', '(blob_t, grad_out, save, pts, c, hidden, nb, leaky, want_rows=False)'),
 'decode_mlp_fwd': ('callable', "(c, blob, pts, precision='f32', wide=None)"),
 'decode_mlp_fwd_train': ('callable', '(c, blob, pts)'),
 'decode_mlp_fwd_wide_train': ('callable', '(c, blob, pts, hidden, nb, leaky)'),
 'decode_range_clear': ('callable', '()'),
 'decode_range_status': ('callable', '(reset=True)'),
 'decode_save_buffer': ('callable', '(total_points, device)'),
 'depth_cloud': ('callable', '(pred, pose, width, height, fov=60.0, dtype=torch.float64)'),
 'dev_ptr': ('callable', "(t, name='tensor', dtype=torch.float32)"),
 'emd_assignment': ('callable', '(a, b, eps_final=None, max_rounds=None)'),
 'f16f8_covers': ('callable', '(grid, lattice, padding=0.1)'),
 'final_fusable': ('callable', '(x, Cout)'),
 'fusion_bwd': ('callable', '(d_out, c_img, c, self_attn, cross_attn, saved, p_drop=0.0, seed=0)'),
 'fusion_dropout_mask': ('callable', '(p_drop, seed, call, which, points, device, d_model=32)'),
 'fusion_fwd': ('callable', '(c_img, c, self_attn, cross_attn)'),
 'fusion_fwd_ids': ('callable', '(finger_ids, finger_feats, c, self_attn, cross_attn, chunk_index=None)'),
 'fusion_fwd_train': ('callable', '(c_img, c, self_attn, cross_attn, p_drop=0.0, seed=0)'),
 'gn_bwd': ('callable',
            '(x, x_stats, low, low_stats, dxn, gamma, groups, eps, want_skip=True, want_low=True, mask_skip=False, mask_low=False, bpart=None)'),
 'gn_conv3d_relu': ('callable',
                    '(x, x_stats, low, low_stats, gamma, beta, groups, packed_w, Cout, eps=1e-05, relu=True, packed_w_bf16x3=None, '
                    'packed_w_f16x3=None, thin_half=False, packed_w_up=None)'),
 'gn_scale_shift': ('callable', '(x_stats, low_stats, C1, C2, B, voxels, gamma, beta, groups, eps, device)'),
 'graph_keepalive': ('callable', '()'),
 'grid_from_channels_last': ('callable', '(grid_cl)'),
 'grid_to_channels_last': ('callable', '(grid)'),
 'is_channels_last_grid': ('callable', '(grid)'),
 'keep_for_graph': ('callable', '(*tensors)'),
 'linear_rows': ('callable', '(x, weight, bias=None)'),
 'mano_bwd': ('callable', '(pose, blob, center_idx, dverts, djoints)'),
 'mano_fwd': ('callable', '(pose, blob, center_idx=9)'),
 'mano_pack': ('callable', '(v_template, shapedirs, betas, posedirs, j_regressor, weights, hands_mean, left=False)'),
 'marching_cubes': ('callable', '(vol, level=None, rescale=None, capacity=None)'),
 'maxpool3d_cl': ('callable', '(x)'),
 'maxpool3d_cl_bwd': ('callable', '(x, dy)'),
 'maxpool3d_cl_bwd_fork': ('callable', '(y, dskip, dpooled, want_absmax=True)'),
 'maxpool3d_cl_stats': ('callable', '(x)'),
 'mc_count': ('callable', '(vol, level=None)'),
 'mc_count_echo': ('callable', '(vol, level, slot)'),
 'mc_count_notify': ('callable', '(vol, level=None)'),
 'mc_echo_arm': ('callable', '(slot)'),
 'mc_echo_release': ('callable', '(slot)'),
 'mc_echo_slot': ('callable', '()'),
 'mc_emit': ('callable', '(vol, ws, rescale=None, capacity=None, token=None, echo=None)'),
 'mise_lattice': ('callable', '(n, box, device, want_ids=True)'),
 'mise_refine': ('callable',
                 '(coarse, level, box, capacity, coarse_known=None, fine=None, known=None, qids=None, qpts=None, count=None, active=None)'),
 'mise_scatter': ('callable', '(fine, ids, vals, known=None)'),
 'pack_decoder': ('callable', "(fc_p_w, fc_p_b, fc_c, blocks, fc_out, fc_out2=None, out=None, transposed=False, precision='f32')"),
 'pack_decoder_wide_t': ('callable', '(fc_p_w, fc_c, blocks, fc_out_w, fc_out2_w=None)'),
 'plane_group': ('callable', '(pis)'),
 'plane_indices': ('callable', "(pts, reso, padding=0.1, planes=('xz', 'xy', 'yz'))"),
 'plane_scatter_mean_bwd': ('callable', '(grad_plane, pi, C)'),
 'plane_scatter_mean_fwd': ('callable', '(feat, pi)'),
 'plane_scatter_mean_multi_bwd': ('callable', '(grad_planes, pis, C)'),
 'plane_scatter_mean_multi_fwd': ('callable', '(feat, pis)'),
 'plane_unet_bwd': ('callable', '(x, net, blob, fwd_ws, dout)'),
 'plane_unet_fwd': ('callable', '(x, net, blob, ws=None)'),
 'plane_unet_pack': ('callable', '(net)'),
 'plane_unet_params': ('callable', '(net)'),
 'plane_unet_supported': ('callable', '(net, H, W)'),
 'plane_unet_workspace': ('callable', '(net, n_img, H, W, fresh=False)'),
 'pointnet_mlp_fused': ('callable', '(p, vi, fc_pos, blocks, fc_c, want_grid=False, weights=None, zeroed_grid=None)'),
 'pointnet_mlp_weights': ('callable', '(fc_pos, blocks, fc_c)'),
 'relu_mask': ('callable', '(dy, y, want_absmax=False)'),
 'resblock_fc': ('callable', '(x1, x2, fc_0, fc_1, shortcut)'),
 'resblock_fc_bwd': ('callable', '(x1, x2, fc_0_w, fc_0_b, fc_1_w, shortcut_w, dout, want_dx2=True)'),
 'resblock_wgrad': ('callable', '(x1, x2, act, dh, dout, has_shortcut)'),
 'resnet_fold_bn': ('callable', '(weight, bn_weight, bn_bias, running_mean, running_var, eps)'),
 'resnet_fwd': ('callable', '(x, net, blob, ws=None)'),
 'resnet_pack': ('callable', '(net)'),
 'resnet_params': ('callable', '(net)'),
 'resnet_supported': ('callable', '(net, n_img, H, W)'),
 'resnet_workspace': ('callable', '(net, n_img, H, W)'),
 'resnet_workspace_floats': ('callable', '(blocks_num, n_img, H, W)'),
 'rows_wgrad': ('callable', '(g, x1, x2=None, relu_x=False, want_bias=True)'),
 'sample_grid': ('callable', '(grid, pts=None, padding=0.1, lattice=None)'),
 'sample_grid_bwd': ('callable', '(grid_shape, pts, grad_feat, padding=0.1)'),
 'sample_grid_bwd_sorted_into': ('callable', '(ggrid_cl, pts, grad_feat, padding=0.1)'),
 'split_decoder_grads': ('callable', '(flat, p_in, hidden=32, c_dim=32, nb=5)'),
 'stat_blocks': ('callable', '(V)'),
 'stream_ptr': ('callable', '()'),
 'tactile_assign': ('callable', '(anchors, success, mode, radius, pts=None, lattice=None, count=None, B=1)'),
 'tactile_unet_bwd': ('callable', '(dout, out, net, scenes, ws)'),
 'tactile_unet_fwd': ('callable', '(x, net, blob, ws=None)'),
 'tactile_unet_pack': ('callable', '(net)'),
 'tactile_unet_params': ('callable', '(net)'),
 'tactile_unet_supported': ('callable', '(net, n_img, H, W)'),
 'tactile_unet_train_fwd': ('callable', '(x, net, scenes=1, momentum=None, ws=None)'),
 'tactile_unet_train_supported': ('callable', '(net, n_img, group, H, W)'),
 'tactile_unet_train_workspace': ('callable', '(net, n_img, group, H, W)'),
 'tactile_unet_workspace': ('callable', '(net, n_img, H, W)'),
 'touch_merge': ('callable',
                 '(ids, anchors, success, mode, radius, nx, box, row_base, capacity, count=None, changed_ids=None, changed_pts=None, n_changed=None, '
                 'workspace=None)'),
 'touch_workspace': ('callable', '(nx, device)'),
 'unet3d_fwd': ('callable', '(x_cl, params, keep, in_stats=None, tile_flags=None)'),
 'unet3d_skip_layers': ('callable', '(B, R, params)'),
 'voxel_pool_max_bwd': ('callable', '(grad_out, argmax, vi)'),
 'voxel_pool_max_fwd': ('callable', '(feat, vi, want_argmax=True)'),
 'voxel_pool_max_sum_bwd': ('callable', '(grad_out, args, vis)'),
 'voxel_pool_max_sum_fwd': ('callable', '(feat, vis, want_argmax=True)'),
 'voxel_pool_mean': ('callable', '(feat, vi)'),
 'voxel_scatter_mean_bwd': ('callable', '(grad_grid, vi, C)'),
 'voxel_scatter_mean_cl_bwd': ('callable', '(grad_grid_cl, vi, C)'),
 'voxel_scatter_mean_cl_fwd': ('callable', '(feat, vi)'),
 'voxel_scatter_mean_fwd': ('callable', '(feat, vi)'),
 'voxel_tile_flags': ('callable', '(vi)'),
 'winding_number': ('callable', '(verts, faces, pts)'),
 'winding_number_scenes': ('callable', '(meshes, pts)')}

# public names added since: none by the split -- the shared helpers of ops/nets2d.py are private to that module; the query of the
# lattice decode's dispatch rule (ops.decode_lattice_form and the names of its results), which the tests of the lattice kernels ask;
# the same query of the wide decoder's launchers (ops.decode_wide_form and the names of its kinds), for tests/test_decode_wide_f64_gpu.py,
# which also reads the backward's dN / dH rows (want_rows of decode_bwd_wide / decode_mlp_bwd_wide); the fuser's launch plan
# (ops.fusion_plan: score form, InstanceNorm kernel, row blocks, capped grids), for tests/test_fusion_f64_gpu.py
NEW_SURFACE = {'LATTICE_FORMS': ('const', "('linear', 'brick', 'staged', 'staged2', 'staged3')"),
               'decode_lattice_form': ('callable', "(R, lattice, padding=0.1, precision='f32', want_contact=False, c_direct=False, C=32)"),
               'WIDE_KINDS': ('const', "('f32', 'bwd', 'f16x3')"),
               'decode_wide_form': ('callable', "(hidden, c_dim, nb, kind='f32', tactile=False, total=0, workspace=False)"),
               'fusion_plan': ('callable', '(B, N, d_model=32, train=False)')}
NEW_PUBLIC = set(NEW_SURFACE)


def _signature(v):
    try:
        return str(inspect.signature(v))
    except ValueError:
        return None


def test_every_recorded_name_is_there_unchanged():
    from vtaco_amd import ops
    for name, (kind, want) in {**SURFACE, **NEW_SURFACE}.items():
        assert hasattr(ops, name), name
        v = getattr(ops, name)
        if kind == "callable":
            assert inspect.isfunction(v) or inspect.isclass(v), name
            assert _signature(v) == want, (name, _signature(v), want)
        else:
            assert repr(v) == want, (name, repr(v), want)


def test_no_other_public_name_appeared():
    from vtaco_amd import ops
    found = set()
    for name, v in vars(ops).items():
        if name.startswith("_") or isinstance(v, types.ModuleType):
            continue
        if inspect.isfunction(v) or inspect.isclass(v):
            if getattr(v, "__module__", "").startswith("vtaco_amd"):
                found.add(name)
        elif re.fullmatch(r"[A-Z][A-Z0-9_]*", name):
            found.add(name)
    assert found - set(SURFACE) == NEW_PUBLIC, sorted(found - set(SURFACE))


def test_private_names_are_the_submodules_objects():
    """``ops._mc_guess`` is the dict ops.mc fills (tests clear it through the package), ``ops._lib`` is the library module, and the
    switches that are assigned at run time live where they are read."""
    import vtaco_amd._lib
    from vtaco_amd import ops
    assert ops._mc_guess is ops.mc._mc_guess
    assert ops.mc.mc_emit.__globals__["_mc_guess"] is ops._mc_guess
    assert ops._lib is vtaco_amd._lib
    assert ops._cl_storage is ops.decode._cl_storage and ops._c is ops._base._c
    assert "GRID_SCATTER_SORTED" in ops.decode_train.decode_bwd.__globals__
    assert ops.decode_train.sample_grid_bwd.__globals__ is ops.decode_train.decode_bwd.__globals__
    assert "_WGRAD_UP" in ops.unet3d.conv3d_wgrad.__globals__


def test_patched_names_have_no_caller_inside_the_package():
    """Tests replace these on the package; that reaches every caller only while no module of ops/ calls them directly."""
    from vtaco_amd import ops
    patched = ("resnet_fwd", "resnet_pack", "resnet_supported", "tactile_unet_fwd", "tactile_unet_train_fwd", "decode_range_status",
               "decode_range_clear")
    root = os.path.dirname(ops.__file__)
    for fn in sorted(os.listdir(root)):
        if fn.endswith(".py"):
            text = open(os.path.join(root, fn)).read()
            for name in patched:
                assert not re.search(r"(?<!def )(?<![\w.])" + name + r"\(", text), (fn, name)
