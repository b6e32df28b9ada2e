"""The drop-in evaluation (fast_path: 0) on the CPU with every evaluation key on: `test()` + `color()` of a `Solver` on the
40 x 40 x 8 scene of tests/test_gpu_epoch_block.py, around the CPU oracle net (oracle/gmfnet_ref.py: model.gmfnet.Net runs on
the GPU only) under freshly initialised weights.  `outputs()` is run twice: by
tools/record_eval_fixtures.py on a checkout of the commit the fixture is recorded from, and by tests/test_calibration_host.py
on the tree under test.  It returns the artefacts decoded (PNG -> pixels, JSON -> its text re-serialised with sorted keys) and
torch's RNG state afterwards, which pins which loaders were iterated, how often and in what order."""
import json
import os

import numpy as np
import torch

SEED = 3407
KEYS = {'test': dict(calibration=1, temperature='fit', spatial='bilateral'), 'color': dict(confidence=1, spatial=1)}
IMAGES = ('0_pic_1.png', '0_pic_2.png', '0_conf_1.png', '0_conf_2.png', '0_pic_1_spatial.png', '0_pic_2_spatial.png')
ARRAYS = ('0_confidence_1.npy', '0_confidence_2.npy')
TEXTS = ('0_calibration.json', '0_spatial.json')


def outputs(golden_dir, tmp):
    from PIL import Image
    from oracle.gmfnet_ref import Net
    from solver.mainsolver import Solver
    from test_gpu_epoch_block import _cfg
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                             # (one summation order in the host's convolutions and products)
    try:
        cfg = _cfg(golden_dir, tmp, 'plain_native_loop', 1)
        cfg.update(device='cpu', fast_path=0)
        cfg['train'] = dict(cfg['train'], index=0)
        cfg['color'] = dict(cfg['color'], index=1, supervised=1, unsupervised=1)
        for sec, val in KEYS.items():
            cfg[sec] = dict(cfg[sec], **val)
        torch.manual_seed(SEED)
        s = Solver(cfg)
        s.dataloader()
        s.cur_model = Net(cfg)
        out = cfg['RESULT_output']
        torch.save(s.cur_model.state_dict(), out + '0_weights.pth')
        s.test()
        s.color()
        r = {'rng_state': torch.get_rng_state().numpy(), 'files': np.array(sorted(os.listdir(out))),
             'test_matrix': s.test_matrix}
        for name in IMAGES:
            r[name] = np.asarray(Image.open(out + name))
        for name in ARRAYS:
            r[name] = np.load(out + name)
        for name in TEXTS:
            r[name] = np.array(json.dumps(json.load(open(out + name)), sort_keys=True))
        return r
    finally:
        torch.set_num_threads(threads)
