"""Minimal KeyFrame / MapPoint / Feature with the reference's observation bookkeeping (src/Keyframe.cpp,
src/MapPoint.cpp) — what Optimizer.LocalBundleAdjustment reads and writes. Poses are 3x4 [R|t] world -> camera.

Kept from the reference: MapPoint::Erase_Observation counts down mObsNum and sets the point bad at <= 1
(src/MapPoint.cpp:57-80); KeyFrame::Erase_MapPointMatch(MapPoint*) clears mvMapPoints only where
Get_IndexInKeyFrame still finds the keyframe among the point's observations (src/Keyframe.cpp:35-43,
src/MapPoint.cpp:207-216). Get_Observations returns the observations in insertion order, which stands for the
std::map<KeyFrame*> order of the reference.
"""
from __future__ import annotations

import numpy as np


class Feature:
    def __init__(self, normal, level: int = 0):
        self.mNormal = np.asarray(normal, np.float64)
        self.mlevel = int(level)


class Camera:
    def __init__(self, mf: float):
        self.mf = float(mf)


class KeyFrame:
    def __init__(self, mlId: int, T_c2w, features, camera: Camera):
        self.mlId = int(mlId)
        self.mlLocalBAKfId = self.mlId             # src/Keyframe.cpp:16-17
        self.mlFixedLocalBAKfId = self.mlId
        self.mvFeatures = list(features)
        self.mvMapPoints = [None] * len(self.mvFeatures)
        self.mCamera = camera
        self.mOrderedCovGraph = []                 # [(weight, KeyFrame)], as GetCovKFrames returns it
        self._T = np.asarray(T_c2w, np.float64).reshape(3, 4).copy()

    def Get_Pose(self):
        return self._T.copy()

    def Set_Pose(self, T):
        self._T = np.asarray(T, np.float64).reshape(3, 4).copy()

    def GetCovKFrames(self):
        return list(self.mOrderedCovGraph)

    def Add_MapPoint(self, mp, idx: int):
        self.mvMapPoints[idx] = mp

    def Erase_MapPointMatch(self, mp):
        idx = mp.Get_IndexInKeyFrame(self)
        if idx >= 0:
            self.mvMapPoints[idx] = None


class MapPoint:
    def __init__(self, mlID: int, pos):
        self.mlID = int(mlID)
        self.mlLocalBAKFId = 0                     # src/MapPoint.cpp:20 (a keyframe with mlId == 0 collects no point)
        self._pos = np.asarray(pos, np.float64).reshape(3).copy()
        self._obs = {}
        self.mObsNum = 0
        self._bad = False

    def Get_Pose(self):
        return self._pos.copy()

    def Set_Pose(self, p):
        self._pos = np.asarray(p, np.float64).reshape(3).copy()

    def IsBad(self):
        return self._bad

    def SetBadFlag(self):
        self._bad = True

    def Add_Observation(self, kf, idx: int):
        if kf in self._obs:
            return
        self._obs[kf] = int(idx)
        self.mObsNum += 1

    def Get_Observations(self):
        return dict(self._obs)

    def Get_IndexInKeyFrame(self, kf):
        return self._obs.get(kf, -1)

    def Erase_Observation(self, kf):
        bad = False
        if kf in self._obs:
            self.mObsNum -= 1
            del self._obs[kf]
            if self.mObsNum <= 1:
                bad = True
        if bad:
            self.SetBadFlag()
