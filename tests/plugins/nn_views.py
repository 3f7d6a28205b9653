"""Model plugin for vector(6) + two image(3,30,30) observations (a camera and a segmentation frame) whose siamese views are
AUGMENTED: every frame is blurred (fixed sigma) and brightened in `forward`, and `get_augmented_encoders` puts one
`RandomChoice` per image in front of its conv stack — salt-and-pepper, uniform noise, blur, or crop(18) -> resize(30).
Written against the plugin API only: with `from torchvision import transforms as T` it loads under the reference."""
import torch
from torch import nn

import algorithm.nn_models as m
from algorithm.utils import image_transforms as T
from algorithm.utils.transform import GaussianNoise, SaltAndPepperNoise


class ModelRep(m.ModelBaseRep):
    def _build_model(self):
        self.blurrer = m.Transform(T.GaussianBlur(3, sigma=1.5))
        self.brightness = m.Transform(T.ColorJitter(brightness=(1.1, 1.1)))
        self.conv_cam = m.ConvLayers(30, 30, 3, 'simple', out_dense_depth=2, output_size=8)
        self.conv_seg = m.ConvLayers(30, 30, 3, 'simple', out_dense_depth=2, output_size=8)
        self.dense = nn.Sequential(nn.Linear(16 + self.obs_shapes[0][0], 8), nn.Tanh())

        crop_resize = lambda: T.Compose([T.RandomCrop(size=(18, 18)), T.Resize(size=(30, 30))])    # noqa: E731
        self.camera_transformers = T.RandomChoice([
            m.Transform(SaltAndPepperNoise(0.2, 0.5)),
            m.Transform(GaussianNoise()),
            m.Transform(T.GaussianBlur(9, sigma=9)),
            m.Transform(crop_resize()),
        ])
        self.segmentation_transformers = T.RandomChoice([
            m.Transform(SaltAndPepperNoise(0.2, 0.5)),
            m.Transform(GaussianNoise()),
            m.Transform(T.GaussianBlur(9, sigma=9)),
            m.Transform(crop_resize()),
        ])

    def _frames(self, obs_list):
        vec, cam, seg = obs_list
        return vec, self.brightness(self.blurrer(cam)), self.brightness(self.blurrer(seg))

    def forward(self, obs_list, pre_action, pre_seq_hidden_state, padding_mask=None):
        vec, cam, seg = self._frames(obs_list)
        state = self.dense(torch.cat([vec, self.conv_cam(cam), self.conv_seg(seg)], dim=-1))
        return state, self._get_empty_seq_hidden_state(state)

    def get_augmented_encoders(self, obs_list):
        _, cam, seg = self._frames(obs_list)
        return self.conv_cam(self.camera_transformers(cam)), self.conv_seg(self.segmentation_transformers(seg))

    def get_state_from_encoders(self, encoders, obs_list, pre_action, pre_seq_hidden_state, padding_mask=None):
        cam, seg = encoders
        return self.dense(torch.cat([obs_list[0], cam, seg], dim=-1))


ModelQ = m.ModelQ
ModelPolicy = m.ModelPolicy
ModelRepProjection = m.ModelRepProjection
ModelRepPrediction = m.ModelRepPrediction
