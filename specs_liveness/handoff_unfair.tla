------------------------------ MODULE handoff_unfair ------------------------------
(* handoff without `fair`: nothing obliges anybody to move, the behaviour that stutters in the first state violates Termination. *)
EXTENDS Naturals

(* --algorithm handoff_unfair
variables token = 0;

process P \in 0..2
begin
  Wait: await token = self;
  Pass: token := token + 1;
end process

end algorithm *)
=============================================================================
