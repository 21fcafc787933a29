"""Drop-in for the reference's training SuperGlue (superglue/models/superglue_train.py:171-307) as far as an inference library can
serve it: the forward signature on a GlueSparse sample, the returned keys ('matches0/1', 'matching_scores0/1', 'loss',
'skip_train') and the forward VALUE of the objective (:289-299), computed by imx_match_loss on the transport matrix of the same
forward.  BatchNorm runs in eval mode, as the folded weights do; there is no backward pass, so `.train()` refuses."""
from pathlib import Path

import torch

from .superglue_test import SuperGlue as _InferenceSuperGlue


class SuperGlue(_InferenceSuperGlue):
    default_config = {
        'descriptor_dim': 256,
        'weights': '',
        'keypoint_encoder': [32, 64, 128, 256],
        'GNN_layers': ['self', 'cross'] * 9,
        'sinkhorn_iterations': 100,
        'match_threshold': 0.2,
    }

    def __init__(self, config, _shared=None):
        named = {**self.default_config, **config}['weights']
        super().__init__({**config, 'weights': None}, _shared)
        self.config['weights'] = named
        if named in ['indoor', 'outdoor', 'mytrain']:                  # (:218-226)
            path = Path(__file__).parent / 'weights/superglue_{}.pth'.format(named)
            model = torch.load(path, map_location='cpu')
            self.load_state_dict(model if named in ['indoor', 'outdoor'] else model['net'])
            print('Loaded SuperGlue model ("{}" weights)'.format(named))

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("image_matching_amd has no backward pass: SuperGlue evaluates the loss of superglue_train.py:289-299 "
                                      "in eval mode only (generate pairs here, train with the reference's module, validate here)")
        return super().train(False)

    def forward(self, data):
        """Run SuperGlue on one sample of GlueSparse as the training loop hands it over (superpoint_glue_train.py:106-112):
        descriptors{0,1} (d,1,N), keypoints{0,1} (1,1,N,2), scores{0,1} (N,1), all_matches (2,1,L), image{0,1} (only .shape)."""
        desc0, desc1 = data['descriptors0'].transpose(0, 1), data['descriptors1'].transpose(0, 1)
        kpts0, kpts1 = torch.reshape(data['keypoints0'], (1, -1, 2)), torch.reshape(data['keypoints1'], (1, -1, 2))
        if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:  # no keypoints (:238-246)
            shape0, shape1 = kpts0.shape[:-1], kpts1.shape[:-1]
            return {
                'matches0': kpts0.new_full(shape0, -1, dtype=torch.int)[0],
                'matches1': kpts1.new_full(shape1, -1, dtype=torch.int)[0],
                'matching_scores0': kpts0.new_zeros(shape0)[0],
                'matching_scores1': kpts1.new_zeros(shape1)[0],
                'skip_train': True
            }
        eng = self._shared.get_engine([self._net])
        m0, m1, ms0, ms1 = eng.superglue(kpts0, torch.transpose(data['scores0'], 0, 1), desc0, data['image0'].shape,
                                         kpts1, torch.transpose(data['scores1'], 0, 1), desc1, data['image1'].shape)
        all_matches = data['all_matches'].permute(1, 0, 2)             # (1, 2, L)
        L_ = all_matches.shape[2]
        cols, n0, n1 = torch.full((1,), L_, dtype=torch.int32, device=eng.device), kpts0.shape[1], kpts1.shape[1]
        if L_ < n0 + n1:       # the library's column buffer is N0 + N1 wide: the rest is padding past n_all
            all_matches = torch.cat([all_matches.to(eng.device, torch.int64), torch.full((1, 2, n0 + n1 - L_), -1, dtype=torch.int64, device=eng.device)], 2)
        loss = eng.match_loss(all_matches, cols)
        return {
            'matches0': m0[0],  # use -1 for invalid match
            'matches1': m1[0],  # use -1 for invalid match
            'matching_scores0': ms0[0],
            'matching_scores1': ms1[0],
            'loss': loss,
            'skip_train': False
        }
