------------------------------ MODULE handoff ------------------------------
(* Three fair processes pass a token once each: every weakly fair behaviour terminates. *)
EXTENDS Naturals

(* --algorithm handoff
variables token = 0;

fair process P \in 0..2
begin
  Wait: await token = self;
  Pass: token := token + 1;
end process

end algorithm *)
=============================================================================
